"""gotennet_amd -- MI355X-native (gfx950) implementation of the GotenNet interaction hot path.

Public surface mirrors the reference package (gotennet/__init__.py:5-10)."""
from .engine import attention_dropout_mask  # noqa: F401
from .gotennet import EQFF, GATA, GotenNet, GotenNetWrapper  # noqa: F401
from .layers import CosineCutoff  # noqa: F401
from .md import MDRun  # noqa: F401

__version__ = "0.1.0"


def __getattr__(name):
    """``gotennet_amd.Relax`` and ``gotennet_amd.CellRelax`` (relax.py) and ``gotennet_amd.NEB`` (neb.py), imported on first use:
    the package itself loads what it loaded before."""
    if name in ("Relax", "CellRelax"):
        from . import relax
        return getattr(relax, name)
    if name in ("NEB", "neb"):
        import importlib
        neb = importlib.import_module(".neb", __name__)
        return neb if name == "neb" else neb.NEB
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
