"""srslte-emane_amd — MI355X-native drop-in for the sample-level hot path of srsLTE's lib/src/phy.

The product is ``csrc/libsrslte_phy_hip.so`` (hand-written HIP for gfx950 behind a C ABI, see
``include/srslte_hip/phy_hip.h``). This package is only the host-side mirror of the reference's operator
interface used by the tests, ``bench.py`` and ``__graft_entry__``: same names, argument meaning and error
behaviour as the ``srslte_*`` calls, numpy arrays in and out, device buffers managed through the C ABI.

There is NO CPU fallback: importing the native handle without a built library raises, and every call needs a GPU.
(The directory name carries a hyphen; import it with ``importlib.import_module("srslte-emane_amd")``.)

One module per group of sections of the header, each with its structs, its rows of the binding table and its objects; every public name
is re-exported here: ``_native`` (the library, ``lib()``, device buffers, shared helpers), ``core``, ``pipelines``, ``dl_ctrl``,
``ul_ctrl``, ``csi``, ``channel``, ``ue_sync``, ``uci_plan``; ``sharding`` is the multi-GPU placement.
"""
from ._native import *  # noqa: F401,F403
from ._native import _check  # noqa: F401
from .channel import *  # noqa: F401,F403
from .core import *  # noqa: F401,F403
from .csi import *  # noqa: F401,F403
from .dl_ctrl import *  # noqa: F401,F403
from .dl_ctrl import _ctrl_tx_in  # noqa: F401
from .pipelines import *  # noqa: F401,F403
from .uci_plan import *  # noqa: F401,F403
from .ue_sync import *  # noqa: F401,F403
from .ul_ctrl import *  # noqa: F401,F403
