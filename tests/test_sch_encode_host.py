"""The transmit side of the link-time drop-in without a GPU: the library exports the transport-block encoder (phy_hip.h) and the reference's
srslte_dlsch_encode2 / srslte_dlsch_encode on top of it (srslte_compat.h), and the structs those two read through - srslte_softbuffer_tx_t and
the soft buffer union of srslte_pdsch_cfg_t - lie in the compat header as in the reference's."""
import ctypes
import os

from _libs import HIP_SO, REF_INC, ROOT, ref_layout, struct_layout

FIELDS = {"srslte_softbuffer_tx_t": ["max_cb", "buffer_b"], "srslte_pdsch_cfg_t": ["softbuffers"]}


def test_the_encoder_entry_points_are_exported():
    lib = ctypes.CDLL(HIP_SO)
    missing = [n for n in ("srslte_hip_sch_enc_create", "srslte_hip_sch_enc_destroy", "srslte_hip_sch_encode", "srslte_dlsch_encode2", "srslte_dlsch_encode")
               if not hasattr(lib, n)]
    assert not missing, missing


def test_transmit_soft_buffer_layout_matches_the_reference():
    ours = struct_layout(FIELDS, ["srslte_hip/srslte_compat.h"], [os.path.join(ROOT, "include")])
    stored = ref_layout({"srslte_softbuffer_tx_t": [], "srslte_pdsch_cfg_t": ["softbuffers"]}, ["srslte/phy/fec/softbuffer.h", "srslte/phy/phch/pdsch_cfg.h"])
    assert {k: ours[k] for k in stored} == stored
    # two members in a struct of the stored size: a uint32_t, then a pointer on its own alignment
    assert (ours["srslte_softbuffer_tx_t.max_cb"], ours["srslte_softbuffer_tx_t.buffer_b"]) == (0, stored["srslte_softbuffer_tx_t"] - ctypes.sizeof(ctypes.c_void_p))
    if os.path.isdir(REF_INC):
        assert struct_layout(FIELDS, ["srslte/phy/fec/softbuffer.h", "srslte/phy/phch/pdsch_cfg.h"], [REF_INC]) == ours
