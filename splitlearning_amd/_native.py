"""Loader for the in-tree native extensions (`_C` and `_C2`, built by `splitlearning_amd.build`)."""
from __future__ import annotations

import importlib
import os

_MODS: dict = {}


def available() -> bool:
    try:
        load()
        return True
    except Exception:
        return False


def _load(name: str):
    mod = _MODS.get(name)
    if mod is not None:
        return mod
    full = f"splitlearning_amd.{name}"
    try:
        mod = importlib.import_module(full)
    except ImportError:
        if os.environ.get("SL_AUTOBUILD", "0") == "1":
            from . import build
            build.build(verbose=False)
            mod = importlib.import_module(full)
        else:
            raise ImportError(f"{full} is not built: run `python -m splitlearning_amd.build`")
    _MODS[name] = mod
    return mod


def load():
    """Import `splitlearning_amd._C`; build it first if the .so is absent and
    SL_AUTOBUILD=1.  Raises ImportError otherwise (no silent fallback)."""
    return _load("_C")


def load2():
    """The same for `splitlearning_amd._C2`, the module of the kernel families added since `_C`'s
    surface was pinned."""
    return _load("_C2")
