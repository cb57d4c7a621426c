"""The multi-row GEMMs' planner (qtts_hip_rows_gemm_plan, host only), pinned
without a GPU for the shipped shapes: the prefill projections of the 0.6B and
1.7B talkers (q|k|v, O, gate|up, down) under the prefill's own dispatch, the
text projection's fc1 (bf16 table by id) and fc2 on k_mgemm, and the 1.7B's
codec-embedding projection over its 3072 table rows, at 17 .. 584 rows with
the workspaces a context of 1024 prompt rows allocates.  The kernel and kz of
every entry are literals, so a planner change shows up as a diff of this file.
"""
import pytest

import qtts
import rows_gemm_ref as G
from rows_gemm_cases import describe, fake_ptrs
from synth_model import PRESETS

ROWS = [17, 24, 64, 65, 73, 97, 300, 584]
ROWS_CAP = 1024
P2, P4 = "k_pgemm<2>", "k_pgemm<4>"
M21, M41, M42, M44 = "k_mgemm<2,1>", "k_mgemm<4,1>", "k_mgemm<4,2>", "k_mgemm<4,4>"

# (kernel, kz, grid) per row count of ROWS
PINS = {
    "0.6b": {
        "qkv": [(P2, 4, [32, 1, 4])] * 6 + [(P4, 4, [16, 3, 4]), (P4, 2, [16, 5, 2])],
        "o": [(P2, 8, [8, 1, 8])] * 6 + [(P4, 8, [4, 3, 8]), (P4, 8, [4, 5, 8])],
        "gate_up": [(P2, 4, [48, 1, 4])] * 6 + [(P4, 4, [24, 3, 4]), (P4, 2, [24, 5, 2])],
        "down": [(P2, 8, [8, 1, 8])] * 6 + [(P4, 8, [4, 3, 8]), (P4, 8, [4, 5, 8])],
        "fc1": [(M21, 8, [128, 1, 8])] * 2 + [(M41, 8, [128, 1, 8])] + [(M41, 4, [128, 2, 4])] * 3
               + [(M42, 2, [64, 5, 2]), (M44, 2, [32, 10, 2])],
        "fc2": [(M21, 8, [64, 1, 8])] * 2 + [(M41, 8, [64, 1, 8])] + [(M41, 8, [64, 2, 8])] * 3
               + [(M41, 2, [64, 5, 2]), (M42, 2, [32, 10, 2])],
    },
    "1.7b": {
        "qkv": [(P2, 8, [32, 1, 8])] * 6 + [(P4, 4, [16, 3, 4]), (P4, 2, [16, 5, 2])],
        "o": [(P2, 8, [16, 1, 8])] * 6 + [(P4, 8, [8, 3, 8]), (P4, 4, [8, 5, 4])],
        "gate_up": [(P2, 4, [96, 1, 4])] * 6 + [(P4, 2, [48, 3, 2]), (P4, 1, [48, 5, 1])],
        "down": [(P2, 8, [16, 1, 8])] * 6 + [(P4, 8, [8, 3, 8]), (P4, 4, [8, 5, 4])],
        "fc1": [(M21, 8, [128, 1, 8])] * 2 + [(M41, 8, [128, 1, 8])] + [(M41, 4, [128, 2, 4])] * 3
               + [(M42, 2, [64, 5, 2]), (M44, 2, [32, 10, 2])],
        "fc2": [(M21, 8, [128, 1, 8])] * 2 + [(M41, 8, [128, 1, 8])] + [(M41, 4, [128, 2, 4])] * 3
               + [(M42, 2, [64, 5, 2]), (M44, 2, [32, 10, 2])],
    },
}
CODEC_EMB_17B = (M44, 1, [16, 48, 1])   # 3072 codec-embedding rows -> the sub-talker's width, no workspace left to split


def workspaces(p):
    """(split floats, plane bf16) a context of ROWS_CAP prompt rows allocates
    (the runtime's sizing: k_mgemm's rule -- 8 columns of every row, at most the
    1024-workgroup grid's tiles -- or k_pgemm's 512 tiles of 128 x 128, and
    three planes of the rows rounded up to the 128-row tile at the widest K)"""
    qkv, ad = (p["NH"] + 2 * p["KV"]) * p["HD"], p["NH"] * p["HD"]
    wide = max(qkv, 2 * p["I"], p["H"], p["TH"])
    part = max(min(8 * max(ROWS_CAP, 64) * wide, 64 * 16 * 4 * 1024), min(512 * 128 * 128, 8 * ROWS_CAP * wide))
    return part, 3 * ((ROWS_CAP + 127) // 128 * 128) * max(p["H"], p["I"], ad)


def roles(p):
    """(name, R, C, form, force): the prefill's projections dispatch as the
    prefill does; the text projection is k_mgemm's"""
    qkv, ad = (p["NH"] + 2 * p["KV"]) * p["HD"], p["NH"] * p["HD"]
    return [("qkv", qkv, p["H"], dict(norm=True), G.F_AUTO),
            ("o", p["H"], ad, dict(epi=G.RESID), G.F_AUTO),
            ("gate_up", 2 * p["I"], p["H"], dict(norm=True, epi=G.SWIGLU), G.F_AUTO),
            ("down", p["H"], p["I"], dict(epi=G.RESID), G.F_AUTO),
            ("fc1", p["TH"], p["TH"], dict(epi=G.BIAS_SILU, src="tab"), G.F_MGEMM),
            ("fc2", p["H"], p["TH"], dict(epi=G.BIAS), G.F_MGEMM)]


def _plan(M, R, Cc, form, force, part, pl):
    cs = G.Case(M, R, Cc, force=force, part=part, planes=pl, **form)
    r = qtts.Kernels.rows_gemm_plan(describe(cs, fake_ptrs(cs)), part, pl, force)
    return None if r is None else (r["kernel"], r["kz"], r["grid"])


@pytest.fixture(autouse=True)
def _no_planner_switches(monkeypatch):
    for k in ("QTTS_HIP_PGEMM_BN", "QTTS_HIP_MGEMM_KZ", "QTTS_HIP_MGEMM_WG"):
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("preset", ["0.6b", "1.7b"])
def test_shipped_projections_keep_their_plan(preset):
    p = PRESETS[preset]
    part, pl = workspaces(p)
    assert (part, pl) == {"0.6b": (8388608, 9437184), "1.7b": (8388608, 18874368)}[preset]
    for name, R, Cc, form, force in roles(p):
        got = [_plan(M, R, Cc, form, force, part, pl) for M in ROWS]
        assert got == PINS[preset][name], (preset, name, got)


def test_codec_embedding_projection_keeps_its_plan():
    p = PRESETS["1.7b"]
    part, pl = workspaces(p)
    assert _plan(p["V"], p["Hs"], p["H"], dict(src="tab"), G.F_MGEMM, part, pl) == CODEC_EMB_17B
    assert p["V"] == 3072 and PRESETS["0.6b"]["H"] == PRESETS["0.6b"]["Hs"]   # (the 0.6B has no such projection)


def test_tile_width_switch_and_argument(monkeypatch):
    """QTTS_HIP_PGEMM_BN moves the prefill's dispatch and leaves a forced width alone"""
    p = PRESETS["1.7b"]
    part, pl = workspaces(p)
    form = dict(epi=G.RESID)
    assert _plan(73, 2048, 2048, form, G.F_AUTO, part, pl)[0] == P2
    assert _plan(73, 2048, 2048, form, G.F_PGEMM256, part, pl) == (P4, 8, [8, 1, 8])
    monkeypatch.setenv("QTTS_HIP_PGEMM_BN", "256")
    assert _plan(73, 2048, 2048, form, G.F_AUTO, part, pl) == (P4, 8, [8, 1, 8])
    assert _plan(73, 2048, 2048, form, G.F_PGEMM128, part, pl) == (P2, 8, [16, 1, 8])
    monkeypatch.setenv("QTTS_HIP_PGEMM_BN", "128")
    assert _plan(300, 2048, 2048, form, G.F_AUTO, part, pl) == (P2, 8, [16, 3, 8])
    # without a workspace nothing splits; without plane scratch the prefill's dispatch is k_mgemm's
    monkeypatch.delenv("QTTS_HIP_PGEMM_BN")
    assert _plan(73, 2048, 2048, form, G.F_AUTO, 0, pl) == (P2, 1, [16, 1, 1])
    assert _plan(73, 2048, 2048, form, G.F_AUTO, part, 0) == (M41, 4, [128, 2, 4])
    assert _plan(73, 2048, 2048, form, G.F_MGEMM, part, pl) == (M41, 4, [128, 2, 4])
    assert _plan(73, 2048, 2048, form, G.F_PGEMM128, part, 0) is None
