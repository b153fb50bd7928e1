"""What to write and how: ``Result`` and its two shortcuts (matchering/results.py:25-46).

A ``Result`` names a file, the sample format inside it and which rendering of the master it
receives: ``use_limiter=True`` the limited one; otherwise the matched track, peak-normalised to the
threshold when ``normalize`` is set and left as it is (possibly above 0 dBFS) when not.
"""

import os

from .audio_io import check_format


def _container_of(path):
    return os.path.splitext(path)[1].lstrip(".").upper()


class Result:
    __slots__ = ("file", "subtype", "use_limiter", "normalize", "delivery")

    def __init__(self, file: str, subtype: str, use_limiter: bool = True, normalize: bool = True, delivery=None):
        container = _container_of(file)
        # same two TypeErrors, in the same order, as the reference raises through soundfile.check_format
        if not check_format(container):
            raise TypeError(f"{container} format is not supported")
        if not check_format(container, subtype):
            raise TypeError(f"{container} format does not have {subtype} subtype")
        self.file, self.subtype = file, subtype
        self.use_limiter, self.normalize = use_limiter, normalize
        # (``delivery``: no counterpart in the reference -- a delivery.Delivery: the rendering is written at a loudness
        # target and / or under a true-peak ceiling, dithered where asked; None: the file is what it was without it)
        if delivery is not None:
            from .delivery import SUBTYPE_BITS, Delivery

            if not isinstance(delivery, Delivery):
                raise TypeError(f"delivery must be a Delivery, got {delivery!r}")
            delivery.check_subtype(subtype)
            if subtype not in SUBTYPE_BITS and subtype not in ("FLOAT", "DOUBLE"):
                raise ValueError(f"Delivery: {subtype} results are not delivered (PCM_16, PCM_24, PCM_32, FLOAT, DOUBLE are)")
            if subtype in SUBTYPE_BITS and container not in ("WAV", "WAVE"):
                # (the device writes the integer samples themselves; another container's codec would quantise them again)
                raise ValueError(f"Delivery: integer deliveries are written to WAVE files, not {container}")
        self.delivery = delivery

    def __repr__(self):
        extra = "" if self.delivery is None else f", delivery={self.delivery!r}"
        return (f"Result({self.file!r}, {self.subtype!r}, use_limiter={self.use_limiter}, "
                f"normalize={self.normalize}{extra})")


def pcm16(file: str, delivery=None) -> Result:
    """16-bit integer samples, limited master."""
    return Result(file, subtype="PCM_16", delivery=delivery)


def pcm24(file: str, delivery=None) -> Result:
    """24-bit integer samples, limited master."""
    return Result(file, subtype="PCM_24", delivery=delivery)
