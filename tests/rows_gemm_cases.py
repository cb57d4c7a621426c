"""The cases of the multi-row GEMMs' tests (test_gpu_rows_gemm.py runs them on
the device, test_rows_gemm_ref.py checks the bound, the planted errors and the
planner on the same cases without one), and the ctypes descriptor of a case.

Shapes are the smallest at which each path can go wrong.  k_mgemm (C % 32,
R % 16): one 16-row tile per workgroup (NW 1) or 2 / 4 of them above 64 rows,
MT 1 / 2 / 4 row tiles by the row count, 64-row chunks on grid.y, four waves
dealing K steps of 32 (C = 32: three of them idle), split-K columns of at
least 8 steps per wave pair (C 512 / 1024 / 2048 give 2 / 4 / 8).  k_pgemm
(rows >= 17, C % 256, R % 32): 128-row tiles with zeroed pad rows, weight
tiles of 128 or 256 rows with the last one clamped to row R - 1, 32-deep K
stages in pairs, split-K columns of at least 8 stages.
"""
import qtts
from rows_gemm_ref import (BIAS, BIAS_SILU, F_AUTO, F_MGEMM, F_PGEMM128, F_PGEMM256, PAD_X, PAD_Y, RESID, STORE,
                           SWIGLU, Case, EPS)

M11, M21, M41, M42, M44, P2, P4 = qtts.RG_NAMES
EPIS = (STORE, BIAS, BIAS_SILU, RESID, SWIGLU)


def _mt(M):
    return M11 if M <= 16 else M21 if M <= 32 else M41


def mgemm_cases():
    out = []
    # the row counts: MT 1 / 2 / 4, then 64-row chunks with a short last chunk; C = 32 (one K step), 64, 288 (nine)
    for i, (M, C) in enumerate([(2, 32), (15, 64), (16, 288), (17, 32), (32, 288), (33, 64), (63, 288), (64, 32),
                                (65, 288), (127, 64), (129, 32)]):
        out.append(Case(M, 80, C, norm=bool(i & 1), kernel=_mt(M)))
    # the smallest R that send 129 rows (three chunks) to 2 and to 4 weight tiles per workgroup
    out.append(Case(129, 2752, 64, kernel=M42))
    out.append(Case(129, 5504, 64, norm=True, kernel=M44))
    # split-K: the workspace exactly kz M R; one float short of kz 4: kz 2
    out.append(Case(40, 80, 512, kernel=M41, kz=2, part=2 * 40 * 80))
    out.append(Case(20, 48, 1024, norm=True, kernel=M21, kz=4, part=4 * 20 * 48))
    out.append(Case(9, 32, 2048, kernel=M11, kz=8, part=8 * 9 * 32))
    out.append(Case(40, 80, 1024, kernel=M41, kz=2, part=4 * 40 * 80 - 1))
    out.append(Case(129, 80, 512, norm=True, kernel=M41, kz=2, part=2 * 129 * 80))
    out.append(Case(129, 2752, 512, kernel=M42, kz=2, part=2 * 129 * 2752))
    out.append(Case(129, 5504, 512, epi=SWIGLU, kernel=M44, kz=2, part=2 * 129 * 5504))
    # every epilogue direct and through k_mgemm_reduce; SwiGLU at R = 16 and at an
    # R whose outputs end inside k_mgemm_reduce's second 256-thread block
    for i, epi in enumerate(EPIS):
        out.append(Case(33, 48, 64, epi=epi, norm=bool(i & 1), kernel=M41))
        out.append(Case(33, 48, 512, epi=epi, norm=not (i & 1), kernel=M41, kz=2, part=2 * 33 * 48))
    out.append(Case(18, 16, 64, epi=SWIGLU, kernel=M21))
    out.append(Case(18, 16, 512, epi=SWIGLU, norm=True, kernel=M21, kz=2, part=2 * 18 * 16))
    out.append(Case(5, 528, 512, epi=SWIGLU, kernel=M11, kz=2, part=2 * 5 * 528))
    out.append(Case(5, 528, 512, epi=RESID, kernel=M11, kz=2, part=2 * 5 * 528))
    # the bf16 table by id (text fc1, the codec embedding projection), id strides 1 and 3, chunks and split
    out.append(Case(20, 48, 64, epi=BIAS_SILU, src="tab", bstride=1, kernel=M21))
    out.append(Case(70, 48, 288, epi=BIAS, src="tab", bstride=3, kernel=M41))
    out.append(Case(70, 48, 512, epi=STORE, src="tab", bstride=3, kernel=M41, kz=2, part=2 * 70 * 48))
    return out


def pgemm_cases():
    out = []
    # rows 17 .. 257 (one short tile, one past a tile, three tiles) x R ending inside a tile; C = 256: 8 stages
    for f, kern, shapes in ((F_PGEMM128, P2, [(17, 32), (127, 96), (128, 128), (129, 160), (257, 96)]),
                            (F_PGEMM256, P4, [(17, 32), (127, 224), (128, 256), (129, 288), (257, 224)])):
        for i, (M, R) in enumerate(shapes):
            out.append(Case(M, R, 256, norm=bool(i & 1), force=f, kernel=kern, planes=True))
    # split-K: C = 512 -> 2, C = 2048 -> 8, and capped at 4 by a workspace short of 8 columns
    out.append(Case(129, 96, 512, force=F_PGEMM128, kernel=P2, kz=2, part=2 * 129 * 96, planes=True))
    out.append(Case(257, 288, 512, norm=True, force=F_PGEMM256, kernel=P4, kz=2, part=2 * 257 * 288, planes=True))
    out.append(Case(17, 32, 2048, norm=True, force=F_PGEMM128, kernel=P2, kz=8, part=8 * 17 * 32, planes=True))
    out.append(Case(129, 160, 2048, force=F_PGEMM256, kernel=P4, kz=4, part=8 * 129 * 160 - 1, planes=True))
    # store, residual and SwiGLU, direct and split, at both tile widths
    for f, kern, R in ((F_PGEMM128, P2, 160), (F_PGEMM256, P4, 288)):
        for i, epi in enumerate((STORE, RESID, SWIGLU)):
            out.append(Case(129, R, 256, epi=epi, norm=not (i & 1), force=f, kernel=kern, planes=True, seed=1))
            out.append(Case(129, R, 512, epi=epi, norm=bool(i & 1), force=f, kernel=kern, kz=2, part=2 * 129 * R,
                            planes=True, seed=1))
    return out


def exact_cases():
    """the exact-plane inputs: one case per kernel and one per split form, C <= 512 but for a single kz = 8 case"""
    E = dict(exact=True)
    return [
        Case(16, 32, 256, kernel=M11, **E),
        Case(16, 48, 512, kernel=M11, kz=2, part=2 * 16 * 48, **E),
        Case(31, 32, 256, kernel=M21, **E),
        Case(31, 48, 512, kernel=M21, kz=2, part=2 * 31 * 48, **E),
        Case(129, 32, 288, kernel=M41, **E),
        Case(129, 48, 512, kernel=M41, kz=2, part=2 * 129 * 48, **E),
        Case(129, 2752, 64, kernel=M42, **E),
        Case(129, 2752, 512, kernel=M42, kz=2, part=2 * 129 * 2752, **E),
        Case(129, 5504, 64, kernel=M44, **E),
        Case(129, 5504, 512, kernel=M44, kz=2, part=2 * 129 * 5504, **E),
        Case(129, 96, 256, force=F_PGEMM128, kernel=P2, planes=True, **E),
        Case(129, 96, 512, force=F_PGEMM128, kernel=P2, kz=2, part=2 * 129 * 96, planes=True, **E),
        Case(257, 96, 256, force=F_PGEMM256, kernel=P4, planes=True, **E),
        Case(257, 96, 512, force=F_PGEMM256, kernel=P4, kz=2, part=2 * 257 * 96, planes=True, **E),
        Case(300, 288, 2048, force=F_PGEMM256, kernel=P4, kz=8, part=8 * 300 * 288, planes=True, **E),
    ]


# force -1: the launcher and kernel the prefill's dispatch takes.  The two
# shipped shapes (a 73-row O projection and a 257-row gate|up of the 1.7B / 0.6B
# talkers, with workspaces as the model sizes them),
# then a 16-row and a 65-row shape with C = 128, which k_pgemm does not cover.
AUTO = [
    Case(73, 2048, 2048, epi=RESID, force=F_AUTO, kernel=P2, kz=8, part=8 * 73 * 2048, planes=True),
    Case(257, 6144, 1024, epi=SWIGLU, norm=True, force=F_AUTO, kernel=P4, kz=4, part=512 * 128 * 128, planes=True),
    Case(16, 48, 128, force=F_AUTO, kernel=M11, planes=3 * 128 * 128),
    Case(65, 48, 128, force=F_AUTO, kernel=M41, planes=3 * 128 * 128),
]

CASES = mgemm_cases() + pgemm_cases()
EXACT = exact_cases()

# What a forced k_pgemm refuses (nothing launched, the output untouched), as
# (what, case, overrides of the descriptor): ldx in floats, x_off in bytes
REFUSED = [
    ("C = 128", Case(129, 96, 128, force=F_PGEMM128, planes=True), {}),
    ("R = 48", Case(129, 48, 256, force=F_PGEMM256, planes=True), {}),
    ("16 rows", Case(16, 96, 256, force=F_PGEMM128, planes=True), {}),
    ("a bias epilogue", Case(129, 96, 256, epi=BIAS, force=F_PGEMM128, planes=True), {}),
    ("ldx % 4 != 0", Case(129, 96, 256, force=F_PGEMM256, planes=True), dict(ldx=256 + 6)),
    ("x misaligned by 4 bytes", Case(129, 96, 256, force=F_PGEMM128, planes=True), dict(x_off=4)),
    ("planes one element short", Case(129, 96, 256, force=F_PGEMM256, planes=3 * 256 * 256 - 1), {}),
]


def describe(cs, ptr, ldx=None, x_off=0):
    """the RowsGemmDesc of a case over the device addresses ptr[name] (A, x |
    table + ids, norm_w, bias, y, part, planes, inv)"""
    d = qtts.RowsGemmDesc()
    d.rows, d.R, d.C, d.A = cs.M, cs.R, cs.C, ptr["A"]
    if cs.src == "x":
        d.src, d.x, d.ldx = 0, ptr["x"] + x_off, cs.C + PAD_X if ldx is None else ldx
    else:
        d.src, d.table, d.ids, d.ids_bstride = 1, ptr["table"], ptr["ids"], cs.bstride
    d.norm_w, d.eps = ptr.get("norm_w") if cs.norm else None, EPS
    d.epi, d.bias = cs.epi, ptr.get("bias") if cs.epi in (BIAS, BIAS_SILU) else None
    d.y, d.ldy = ptr["y"], cs.nout + PAD_Y
    d.part, d.part_elems = (ptr.get("part"), cs.part) if cs.part else (None, 0)
    d.planes, d.plane_elems = (ptr.get("planes"), cs.plane_elems) if cs.plane_elems else (None, 0)
    d.inv = ptr.get("inv")
    return d


def fake_ptrs(cs):
    """stand-in addresses (256-byte aligned, never dereferenced) for the host-only planner"""
    names = ["A", "x", "table", "ids", "norm_w", "bias", "y", "part", "planes", "inv"]
    return {k: (i + 1) << 24 for i, k in enumerate(names)}


def plan(cs, **over):
    """the planner's answer for the case (host only): (kernel name, kz) or None"""
    p = qtts.Kernels.rows_gemm_plan(describe(cs, fake_ptrs(cs), **over), cs.part, cs.plane_elems, cs.force)
    return None if p is None else (p["kernel"], p["kz"])
