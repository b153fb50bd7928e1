"""tests/emu/build.py for the tests: imported by path, once (tests/emu is a folder of C++ sources, not a package).

``load(name)`` is the ``ctypes.CDLL`` of an emulation unit, built first where it is out of date; ``build_driver(name, out,
extra_flags)`` the unit's stand-alone program."""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location(
    "mgx_emu_build", os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu", "build.py"))
_module = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_module)

UNITS, build, build_driver, load = _module.UNITS, _module.build, _module.build_driver, _module.load
