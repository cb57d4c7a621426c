"""k_convh<Kw,2> / k_convh<Kw,4> (k_convh.hip: the codec convs on one bf16
plane per operand) through qtts_hip_xgemm_case / _seg_case with force_path 6 /
7, against the float64 reference of xgemm_ref.py computed from the fp32 inputs.

Bound per output element: b_acc + b_snake + b_round, pushed through the
epilogue as xgemm_ref.epilogue does.  b_acc and the SnakeBeta term are
test_gpu_xgemm.py's (2e-6 sum |a||b'| + 1e-6, + sum |a| d_snake(b)).
b_round = (2^-8 + 2^-18) sum |a||b'|: each operand rounded to the nearest bf16
carries a relative error <= 2^-9, so a product <= 2 * 2^-9 + 2^-18.  Derived,
not tuned.

Every case runs a second time with weights and inputs drawn on the bf16 grid
and no SnakeBeta prologue: nothing is rounded then, and b_acc alone must hold.
That run is the sharp one: a dropped tap, a wrong stage tail, a wrong swizzle
or a wrong segment base all pass the looser bound's 0.4 % and none passes this.
"""
from dataclasses import replace

import numpy as np
import pytest

import qtts
import xgemm_ref as X
from attn_ref import rne_bf16, widen
from xgemm_cases import CASES as EXACT_CASES, conv, describe, fake_ptrs, layout, lin, shipped, tconv, RES, SNK

H2, H4 = 6, 7                     # QTTS_XP_CONVH2 / QTTS_XP_CONVH4
C_ROUND = 2.0 ** -8 + 2.0 ** -18

# (spec, segments).  Stages hold 32 channels: 48 (and 96 on two splits) end in a 16-channel stage.
CONVH = [
    (conv(H2, 1, 70, 16, 7, 1, snake=True, hist=True), 1),             # the decoder's last conv: one output row
    (conv(H2, 96, 130, 48, 7, 3, e=SNK, hist=True), 3),                # partial row tile, two column tiles, tail stage
    (conv(H2, 96, 70, 32, 3, 9, e=RES, hist=True, snake=True), 1),
    (conv(H2, 64, 130, 16, 2, 1, hist=True), 1),
    (conv(H2, 96, 130, 48, 1, e=RES), 1),
    (conv(H2, 96, 130, 96, 7, 1, hist=True, splits=2, part=2 * 96 * 130), 1),       # 48 channels per split
    (conv(H2, 65, 70, 64, 3, 3, e=SNK, snake=True, splits=2, part=2 * 3 * 65 * 70), 3),
    (tconv(H2, 96, 70, 32, 8, 4, hist=True), 1),                       # stride 4, kernel 8: four phases on grid z
    (tconv(H2, 65, 130, 96, 8, 4, snake=True, splits=2, part=2 * 4 * 65 * 130), 1),
    (conv(H4, 96, 260, 48, 7, 9, e=SNK, hist=True, snake=True), 1),
    (conv(H4, 1, 70, 16, 7, 1), 1),
    (conv(H4, 64, 260, 32, 3, 3, e=RES, hist=True), 3),
    (conv(H4, 96, 260, 96, 2, 1, hist=True, splits=2, part=2 * 96 * 260), 1),
    (conv(H4, 65, 70, 16, 1), 1),
    (tconv(H4, 63, 260, 48, 8, 4, hist=True), 1),
]
REFUSED = [lin(H2, 64, 64, 128), lin(H4, 64, 64, 128),
           conv(H2, 64, 128, 3072, 1, snake=True), conv(H4, 64, 128, 3072, 1, snake=True)]   # > CB_SNAKE_MAX channels


def _on_grid(a):
    return widen(rne_bf16(np.asarray(a, np.float32))).reshape(a.shape).astype(np.float32)


def _segments(sp, nseg, grid):
    """per segment (inputs, out, bound): shared weights and parameters, each
    segment its own input row block, margins included"""
    d0 = X.make_inputs(sp)
    segs = []
    for s in range(nseg):
        d = dict(d0)
        if s:
            own = X.make_inputs(replace(sp, seed=100 + s))
            d.update({k: own[k] for k in ("x", "c0") if k in own})
        if grid:
            d["w"], d["x"] = _on_grid(d["w"]), _on_grid(d["x"])
        acc, b_acc = X.accumulate(sp, d)
        if not grid:
            x = d["x"].astype(np.float64)
            if sp.snake:
                x = X.snake64(x, d["sa"][:, None], d["sb"][:, None])
            for ph in range(sp.stride):
                b_acc[:, ph::sp.stride] += C_ROUND * X.gather(sp, np.abs(X.wmat(sp, d["w"], ph)), np.abs(x))
        segs.append((d,) + X.epilogue(sp, d, acc, b_acc))
    return segs


def _run(gpu, sp, segs):
    """one launch over the segments: (ran, C after [nseg][crows][ldc], C before)"""
    import torch
    lo, nseg, nan = layout(sp), len(segs), np.float32(np.nan)
    keep, ptr = [], {}

    def put(name, a, off=0):
        keep.append(torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(gpu))
        ptr[name] = keep[-1].data_ptr() + 4 * off

    d0 = segs[0][0]
    if sp.kind == "lin":
        put("A", np.pad(d0["A"], ((0, 0), (0, 4))))
        put("B", np.pad(d0["W"], ((0, 0), (0, 4))))
    else:
        xs = np.stack([s[0]["x"] for s in segs]).astype(np.float32)
        xs[:, :, :X.LM + sp.tmin] = nan            # left of the history and right of the row: an over-read shows
        xs[:, :, X.LM + sp.N:] = nan
        put("A", d0["w"])
        put("B", xs, X.LM)
    for k in ("sa", "sb", "bias", "ea", "eb"):
        if k in d0:
            put(k, d0[k])
    C0 = np.full((nseg, lo["crows"], lo["ldc"]), X.SENTINEL, np.float32)
    for s, (d, _, _) in enumerate(segs):
        if "c0" in d:
            C0[s, :d["c0"].shape[0], :d["c0"].shape[1]] = d["c0"]
    put("C", C0)
    desc = describe(sp, ptr)
    if nseg == 1:
        ran = qtts.Kernels.xgemm_case(desc, sp.part, sp.force)
    else:
        ran = qtts.Kernels.xgemm_seg_case(desc, nseg, sp.ci * lo["ldb"], lo["crows"] * lo["ldc"], sp.part, sp.force)
    torch.cuda.synchronize()
    return ran, keep[-1].cpu().numpy(), C0


@pytest.mark.gpu
@pytest.mark.parametrize("grid", [False, True], ids=["rounded", "grid-exact"])
@pytest.mark.parametrize("sp,nseg", CONVH, ids=[f"{sp.id()}-seg{n}" for sp, n in CONVH])
def test_convh(gpu, sp, nseg, grid):
    if grid:
        sp = replace(sp, snake=False)
    segs = _segments(sp, nseg, grid)
    ran, C, C0 = _run(gpu, sp, segs)
    assert ran == (sp.path, sp.splits), (ran, sp.id())
    R, Cn = segs[0][1].shape
    worst = 0.0
    for s, (_, ref, bound) in enumerate(segs):
        got = C[s, :R, :Cn].astype(np.float64)
        assert np.all(np.isfinite(got)), (sp.id(), s)
        err = np.abs(got - ref)
        worst = max(worst, float(np.max(err / bound)))
        assert np.all(err <= bound), (sp.id(), s, worst, np.argwhere(~(err <= bound))[:4])
    print(f"err / bound  {qtts.XP_NAMES[sp.path]} {'grid-exact' if grid else 'rounded':10s} {worst:.4f}  {sp.id()} seg{nseg}")
    mask = np.ones(C.shape, bool)
    mask[:, :R, :Cn] = False                       # beside and between the segments: untouched, bit for bit
    assert np.array_equal(C.view(np.uint32)[mask], C0.view(np.uint32)[mask]), sp.id()


@pytest.mark.gpu
@pytest.mark.parametrize("sp", REFUSED, ids=[sp.id() for sp in REFUSED])
def test_convh_refuses_what_it_does_not_cover(gpu, sp):
    ran, C, C0 = _run(gpu, sp, [(X.make_inputs(sp), None, None)])
    assert ran is None
    assert np.array_equal(C.view(np.uint32), C0.view(np.uint32))


def test_default_descriptor_never_plans_convh():
    """host only: the planner answers 6 / 7 for no default (exact) descriptor --
    the kernel tests' cases and every contraction of a 1.7B decode -- and
    accepts both ids as force_path on a conv"""
    specs = [replace(sp, force=-1) for sp in EXACT_CASES]
    specs += [sp for T in (1, 16, 128) for _, sp in shipped(T)]
    for sp in specs:
        plan = qtts.Kernels.xgemm_plan(describe(sp, fake_ptrs(sp)), sp.part, -1)
        assert plan is not None and plan[0] not in (H2, H4), (sp.id(), plan)
    for sp, _ in CONVH:
        assert qtts.Kernels.xgemm_plan(describe(sp, fake_ptrs(sp)), sp.part, sp.force) == (sp.path, sp.splits), sp.id()
