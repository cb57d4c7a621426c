"""The multi-row GEMMs' reference, bound and exact-plane inputs, checked without
a device on the very inputs test_gpu_rows_gemm.py runs.

(a) The kernels' arithmetic restated in numpy (rows_gemm_ref.model: fp32 norm,
    three bf16 planes, plane products summed in float64 or in fp32 split
    column by split column) passes the check of every case: the bound is not
    tighter than a correct kernel, and the exact-plane cases are exact.
(b) Each planted error fails the check of every case it applies to (the GPU
    test fails on a single element): third plane dropped (the exact-plane
    check only: the bound cannot see it, which (c) measures), second plane
    dropped, last K stage skipped, one split column omitted, gate and up
    swapped in a quad, a row past R - 1 written from the clamped row, one pad
    row's contribution added to row M - 1.
(c) What the 2e-6 bound does and does not see, measured as the issue states it.
(d) The host-only planner (qtts_hip_rows_gemm_plan) reports for every case
    the kernel and kz the case was written for, refuses what the refusal cases
    say, and rejects bad descriptors.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import qtts
import rows_gemm_ref as G
from conftest import ROOT
from rows_gemm_cases import AUTO, CASES, EXACT, REFUSED, describe, fake_ptrs, plan

SMALL_AUTO = [cs for cs in AUTO if cs.R * cs.C <= 1 << 20]
ALL = CASES + EXACT + SMALL_AUTO


def _fails(cs, d, ref, bound, mutate):
    y0 = G.y_buffer(cs, d)
    ok, ratio, why = G.check(cs, G.model(cs, d, mutate), y0, ref, bound)
    return (not ok), ratio, why


@pytest.mark.parametrize("cs", ALL, ids=[cs.id() for cs in ALL])
def test_models_pass_and_planted_errors_fail(cs):
    d, ref, bound = G.reference(cs)
    y0 = G.y_buffer(cs, d)
    for fp32 in (False, True):
        ok, ratio, why = G.check(cs, G.model(cs, d, fp32=fp32), y0, ref, bound)
        assert ok, (cs.id(), "fp32" if fp32 else "float64", ratio, why)
    muts = ["last_stage", "clamped_row", "pad_row"]
    if cs.src == "x":                 # (a bf16 table row has no second plane)
        muts.append("drop2")
    if cs.exact:
        muts.append("drop3")
    if cs.kz > 1:
        muts.append("split_column")
    if cs.epi == G.SWIGLU:
        muts.append("gate_up")
    for m in muts:
        failed, ratio, why = _fails(cs, d, ref, bound, m)
        assert failed, (cs.id(), m, ratio)


def test_exact_cases_are_what_they_claim():
    """one exact-plane case per kernel and per split form, C <= 512 but for one
    kz = 8 case; a dropped third plane changes most outputs"""
    seen = {(cs.kernel, cs.kz > 1) for cs in EXACT}
    assert seen == {(k, s) for k in qtts.RG_NAMES for s in (False, True)}
    assert [cs for cs in EXACT if cs.C > 512] == [cs for cs in EXACT if cs.kz == 8] and sum(cs.kz == 8 for cs in EXACT) == 1
    for cs in EXACT:
        d, ref, bound = G.reference(cs)
        got = G.model(cs, d, "drop3")[:cs.M, :cs.nout].astype(np.float64)
        frac = float(np.mean(got != ref))
        print(f"dropped third plane changes {frac:.2f} of the outputs  {cs.id()}")
        assert frac > 0.5, (cs.id(), frac)


def test_what_the_bound_sees():
    """standard-normal x, bf16 weights of scale 1/sqrt(K), 64 x 2048 x 64: a
    dropped third plane stays inside the bound (0.21 of it at most when
    measured for the issue), a dropped second plane is 100 times outside"""
    cs = G.Case(64, 64, 2048, kernel="k_mgemm<4,1>")
    d, ref, bound = G.reference(cs, keep=False)
    y0 = G.y_buffer(cs, d)
    ok3, r3, _ = G.check(cs, G.model(cs, d, "drop3"), y0, ref, bound)
    ok2, r2, _ = G.check(cs, G.model(cs, d, "drop2"), y0, ref, bound)
    print(f"err / bound  third plane dropped {r3:.3f}, second plane dropped {r2:.1f}")
    assert ok3 and r3 < 0.5
    assert not ok2 and r2 > 20


def test_cases_cover_what_they_were_written_for():
    both = CASES + EXACT
    for k in qtts.RG_NAMES:
        assert any(cs.kernel == k and cs.kz == 1 for cs in both), k
        assert any(cs.kernel == k and cs.kz > 1 for cs in both), k
    mg = [cs for cs in CASES if cs.kernel.startswith("k_mgemm")]
    for epi in range(5):
        assert any(cs.epi == epi and cs.kz == 1 for cs in mg) and any(cs.epi == epi and cs.kz > 1 for cs in mg), epi
    assert {cs.bstride for cs in mg if cs.src == "tab"} == {1, 3}
    assert {cs.kz for cs in mg} == {1, 2, 4, 8}
    pg = [cs for cs in CASES if cs.kernel.startswith("k_pgemm")]
    for kern in ("k_pgemm<2>", "k_pgemm<4>"):
        assert {cs.M for cs in pg if cs.kernel == kern} >= {17, 127, 128, 129, 257}, kern
        for epi in (G.STORE, G.RESID, G.SWIGLU):
            for split in (False, True):
                assert any(cs.kernel == kern and cs.epi == epi and (cs.kz > 1) == split for cs in pg), (kern, epi, split)
        assert {cs.norm for cs in pg if cs.kernel == kern} == {False, True}
    assert {cs.R for cs in pg if cs.kernel == "k_pgemm<2>"} >= {32, 96, 128, 160}
    assert {cs.R for cs in pg if cs.kernel == "k_pgemm<4>"} >= {32, 224, 256, 288}
    assert {cs.kz for cs in pg} == {1, 2, 4, 8}


# ---------------------------------------------------------------- the planner, host only
@pytest.fixture(autouse=True)
def _no_planner_switches(monkeypatch):
    for k in ("QTTS_HIP_PGEMM_BN", "QTTS_HIP_MGEMM_KZ", "QTTS_HIP_MGEMM_WG"):
        monkeypatch.delenv(k, raising=False)


def test_planner_reports_every_case_as_written():
    for cs in CASES + EXACT + AUTO:
        assert plan(cs) == (cs.kernel, cs.kz), (cs.id(), plan(cs))


@pytest.mark.parametrize("what,cs,over", REFUSED, ids=[r[0] for r in REFUSED])
def test_planner_refuses(what, cs, over):
    assert plan(cs, **over) is None, what
    # the same shape is k_mgemm's where k_mgemm covers it
    covered = cs.M >= 2 and not over
    from dataclasses import replace
    assert (plan(replace(cs, force=G.F_MGEMM), **over) is not None) == covered, what


def test_planner_rejects_bad_descriptors():
    lib = qtts.lib()
    cs = CASES[0]

    def rc(force=0, out=True, **kw):
        d = describe(cs, fake_ptrs(cs))
        for k, v in kw.items():
            setattr(d, k, v)
        p = qtts.RowsGemmPlan()
        return lib.qtts_hip_rows_gemm_plan(C.byref(d), 0, 0, force, C.byref(p) if out else None)

    assert rc() == 0
    assert lib.qtts_hip_rows_gemm_plan(None, 0, 0, 0, C.byref(qtts.RowsGemmPlan())) == -1
    assert rc(out=False) == -1
    for bad in (dict(A=None), dict(x=None), dict(y=None), dict(rows=0), dict(R=0), dict(C=0), dict(epi=5), dict(epi=-1),
                dict(src=2), dict(src=1), dict(epi=1), dict(epi=2), dict(ldy=cs.R - 1), dict(ldx=cs.C - 4)):
        assert rc(**bad) == -1, bad
        d = describe(cs, fake_ptrs(cs))
        for k, v in bad.items():
            setattr(d, k, v)
        assert lib.qtts_hip_rows_gemm_case(C.byref(d), 0, None, None) == -1, bad   # (before any device work)
    assert rc(force=3) == -1 and rc(force=-2) == -1
    assert rc(rows=1) == 1            # (one row is the GEMV's)


def test_library_exports_and_binding_declares_the_entries():
    lib = qtts.lib()
    names = ["qtts_hip_rows_gemm_plan", "qtts_hip_rows_gemm_case"]
    assert all(hasattr(lib, s) for s in names) and set(names) <= set(qtts.EXPORTS)
    assert lib.qtts_hip_rows_gemm_plan.argtypes == [C.POINTER(qtts.RowsGemmDesc), C.c_size_t, C.c_size_t, C.c_int,
                                                    C.POINTER(qtts.RowsGemmPlan)]
    assert lib.qtts_hip_rows_gemm_case.argtypes == [C.POINTER(qtts.RowsGemmDesc), C.c_int,
                                                    C.POINTER(qtts.RowsGemmPlan), C.c_void_p]
    assert callable(qtts.Kernels.rows_gemm_plan) and callable(qtts.Kernels.rows_gemm_case)
    assert qtts.RG_NAMES == G.RG_NAMES
    # the descriptor, the plan and the kernel numbers mirror the header field for field
    txt = open(os.path.join(ROOT, "include", "qtts_hip.h")).read()
    for ctype, mirror in (("qtts_rows_gemm_desc_t", qtts.RowsGemmDesc), ("qtts_rows_gemm_plan_t", qtts.RowsGemmPlan)):
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % ctype, txt).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = []
        for decl in body.split(";"):
            parts = [p.strip() for p in decl.split(",") if p.strip()]
            fields += [re.sub(r"^.*[\s\*]", "", p) for p in parts]
        assert fields == [f[0] for f in mirror._fields_], fields
    enum = dict(re.findall(r"QTTS_RG_(\w+) = (\d)", txt))
    assert [f"k_{k[:5].lower()}<{k[6:].replace('_', ',')}>" for k in sorted(enum, key=enum.get)] == qtts.RG_NAMES
    for doc in ("INTEGRATION.md",):
        body = open(os.path.join(ROOT, doc)).read()
        assert all(s in body for s in names), doc
