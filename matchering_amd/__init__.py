"""matchering_amd -- MI355X-native mastering core behind the matchering API.

Public names mirror matchering/__init__.py:31-36 (``log``, ``Result``, ``pcm16``,
``pcm24``, ``Config``, ``process``, ``load``, ``check``); the DSP of
``matchering.stages.main`` runs as hand-written HIP kernels (libmgx.so).
"""

__version__ = "0.1.0"
__reference_version__ = "2.0.6"

from .log import set_handlers as log  # noqa: F401
from .results import Result, pcm16, pcm24  # noqa: F401
from .config import Config, LimiterConfig  # noqa: F401
from .core import process  # noqa: F401
from .audio_io import load  # noqa: F401
from .checker import check  # noqa: F401
from .batch import master_many, process_batch  # noqa: F401  (no counterpart in the reference)
from .profile import ReferenceProfile  # noqa: F401  (nor this: a reference analysed once, kept without its audio)
from .loudness import Loudness, measure  # noqa: F401  (nor this: BS.1770-4 loudness and true peak of frames in HBM)
from .delivery import Delivered, Delivery, NoiseShaper, TruePeakLimiter  # noqa: F401  (nor this: results at a loudness target, under a true-peak ceiling, dithered)
from .qc import Audit, AuditLimits, audit  # noqa: F401  (nor this: the quality-control pass over tracks, renderings and written files)
from .visuals import Overview, Spectrogram, Visuals, VisualsRequest, overview, spectrogram  # noqa: F401  (nor this: waveform overview and spectrogram of frames in HBM)
from .eq import MatchingEq, ToneBand  # noqa: F401  (nor this: strength, boost / cut caps, minimum phase and tone controls for the matching EQ)
from .repair import ClipRepair, Repaired, repair_clipping  # noqa: F401  (nor this: a clipped target's short flat tops rebuilt in HBM before it is mastered)
