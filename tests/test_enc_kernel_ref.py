"""enc_kernel_ref.py's bounds tell a right kernel from a wrong one, on a CPU
box: k_econv's arithmetic restated in numpy (run_model: three bf16 planes of
both operands, the six kept products, fp32 accumulation per MFMA, the split-K
order, the kernel's own index arithmetic) passes every case of
enc_kernel_cases.py, and each mutant of it fails at least one.  A dropped
third-order product (a1b3, a2b2, a3b1) is below the bound from K = 128 on: it
passes those cases and fails its exact-plane instrument.  The same for the
small kernels' bounds with fp32 restatements of them."""
import numpy as np
import pytest

import enc_kernel_cases as CS
import enc_kernel_ref as E
from enc_kernel_ref import f32

# the ROWS cross product is large: the mutants run on one case per (K, epilogue)
MUTANT_CASES = CS.GENERIC + CS.NOT_ROWS + [CS.ROWS_GELU_LS] + [cv for cv in CS.ROWS if cv.M == 48 and cv.lin == (65,)]


def _passes(cv, **kw):
    lo = E.layout(cv, E.reference(cv)[0])
    try:
        E.check(cv, lo, E.run_model(cv, lo, **kw))
        return True
    except AssertionError:
        return False


@pytest.mark.parametrize("cv", CS.CASES, ids=[cv.id() for cv in CS.CASES])
def test_faithful_model_passes(cv):
    lo = E.layout(cv, E.reference(cv)[0])
    assert E.plan_model(cv, lo) == (cv.rows, cv.kz)
    ratio = E.check(cv, lo, E.run_model(cv, lo))
    assert ratio < 0.5      # the bound is not at the model's own error: mutants are told apart with room


def test_table_cases_reach_the_branches_they_are_for():
    by = {cv.name: cv for cv in CS.GENERIC}
    assert by["stft"].lin[-1] == by["stft"].padl + 1                       # the shortest the launcher accepts
    assert ((by["res2net-d2"].K + 31) // 32) % by["res2net-d2"].kz == 1    # uneven split
    assert by["asp"].K % 8 == 4 and by["seanet-first"].K < 32
    for cv in CS.STRIDED:                                                  # reads past lin on the right
        assert (cv.lout[0] - 1) * cv.stride - cv.padl + cv.kw - 1 >= cv.lin[0]
    assert ((by["cap-16"].K + 31) // 32) // 4 > 16
    assert {cv.kz for cv in CS.ROWS} == {1, 2, 4} and {cv.rows for cv in CS.ROWS} == {1}
    assert all(cv.rows == 0 for cv in CS.NOT_ROWS)


MUTANTS = ["tap", "reflect", "replicate", "dil", "stride", "x2", "elu_order", "last_step", "bias2", "vec_order",
           "res_t", "last_row", "last_col"]


@pytest.mark.parametrize("mut", MUTANTS)
def test_mutant_fails_a_case_of_the_table(mut):
    killed = [cv.id() for cv in MUTANT_CASES if not _passes(cv, mut=(mut,))]
    print(f"{mut}: {len(killed)} cases fail, e.g. {killed[:2]}")
    assert killed, mut


@pytest.mark.parametrize("drop", [(0, 1), (1, 0)], ids=["a1b2", "a2b1"])
def test_dropped_second_order_product_fails_the_bound(drop):
    killed = [cv.id() for cv in MUTANT_CASES if not _passes(cv, drop=drop)]
    assert len(killed) >= len(MUTANT_CASES) // 2, killed      # about 2^-16 relative: far above 2e-6 everywhere


@pytest.mark.parametrize("drop,ins", [((0, 2), "B"), ((1, 1), "C"), ((2, 0), "A")], ids=["a1b3", "a2b2", "a3b1"])
def test_dropped_third_order_product_passes_the_bound_and_fails_its_instrument(drop, ins):
    # Each term loses about 2^-16 |w x| with a random sign, so the loss grows as
    # sqrt(K) while the bound's sum |w||x| grows as K: from four K-steps on
    # (K >= 128, every split-K case among them) the bound cannot see it.  Below
    # that the bound may or may not catch it, and nothing is claimed.
    wide = [cv for cv in MUTANT_CASES if cv.K >= 128]
    assert len(wide) >= 12 and all(_passes(cv, drop=drop) for cv in wide)
    for cv in CS.EXACT:
        assert _passes(cv, drop=drop) == (cv.exact != ins), (cv.id(), drop)


def test_full_three_plane_inputs_are_no_instrument():
    """three planes on both sides: the dropped products are nonzero, so the
    builder's own assertions refuse the inputs (why there are three instruments)"""
    from dataclasses import replace
    cv = replace(CS.EXACT[3], exact="full", name="full")
    with pytest.raises(AssertionError):
        E.exact_operands(cv, E.make_inputs(cv))


def test_split_order_does_not_matter_on_the_instruments():
    for cv in CS.EXACT:
        lo = E.layout(cv, E.reference(cv)[0])
        for kz in (1, 2, 3):
            E.check(cv, lo, E.run_model(cv, lo, kz=kz))


# ------------------------------------------------------------------ small kernels
def _sum32(a, axis=-1):
    return np.sum(f32(a), axis=axis, dtype=np.float32)


def _stats32(x, L, one_pass=False, clamp=True):
    x = f32(x)[:, :L]
    m = np.float32(1.0 / L)
    mean = _sum32(m * x)
    if one_pass:
        v = _sum32(m * x * x) - mean * mean
    else:
        v = _sum32(m * f32(x - mean[:, None]) ** 2)
    return mean, np.sqrt(np.maximum(v, np.float32(1e-12)) if clamp else v)


def _pool32(x, a, L, sub_max=True):
    x, a = f32(x)[:, :L], f32(a)[:, :L]
    mx = a.max(-1, keepdims=True) if sub_max else np.float32(0)
    with np.errstate(over="ignore", invalid="ignore"):
        e = np.exp(f32(a - mx))
        w = f32(e * f32(np.float32(1) / _sum32(e)[:, None]))
        mean = _sum32(w * x)
        v = _sum32(w * f32(x - mean[:, None]) ** 2)
    return mean, np.sqrt(np.maximum(v, np.float32(1e-12)))


def _within(got, ref, bound):
    got = np.asarray(got, np.float64)
    return bool(np.all(np.isfinite(got)) and np.all(np.abs(got - ref) <= bound))


@pytest.mark.parametrize("Cn", CS.STAT_C)
def test_stats_bounds(Cn):
    x, lg, lens = CS.stats_inputs(Cn)
    one_pass_ok, nomax_ok = True, True
    for b, L in enumerate(lens):
        mean, std, b_mean, b_std = E.asp_stats_ref(x[b][:, :L])
        assert np.all(np.isfinite(b_std)) and std[1] == 1e-6               # the constant channel
        m32, s32 = _stats32(x[b], L)
        assert _within(m32, mean, b_mean) and _within(s32, std, b_std)
        assert _within(m32, *E.mean_ref(x[b][:, :L]))
        m1, s1 = _stats32(x[b], L, one_pass=True)
        one_pass_ok &= _within(s1, std, b_std)
        pm, ps, pbm, pbs = E.asp_pool_ref(x[b][:, :L], lg[b][:, :L])
        g = _pool32(x[b], lg[b], L)
        assert _within(g[0], pm, pbm) and _within(g[1], ps, pbs), (b, L)
        g = _pool32(x[b], lg[b], L, sub_max=False)
        nomax_ok &= _within(g[0], pm, pbm) and _within(g[1], ps, pbs)
    assert not one_pass_ok, "a one-pass variance passes"
    assert not nomax_ok, "a softmax without the max subtraction passes"


@pytest.mark.parametrize("nf,nm", CS.MEL)
def test_mel_bound(nf, nm):
    spec, fb, flo, fhi, T = CS.mel_inputs(nf, nm)
    noclamp_ok = True
    for b in range(len(T)):
        ref, bound, acc = E.mel_ref(spec[b][:, :T[b]], fb, flo, fhi)
        assert np.all(acc[1] == 0.0) and np.all(acc[2] < 1e-5) and np.all(acc[2] > 0)
        s = f32(spec[b][:, :T[b]])
        mag = np.sqrt(f32(f32(s[:nf] * s[:nf]) + f32(s[nf:] * s[nf:])) + np.float32(1e-9))
        a32 = np.stack([_sum32(fb[m, flo[m]:fhi[m], None] * mag[flo[m]:fhi[m]], 0) for m in range(nm)])
        assert _within(np.log(np.maximum(a32, np.float32(1e-5))), ref, bound)
        with np.errstate(divide="ignore"):
            noclamp_ok &= _within(np.log(a32), ref, bound)
        assert not _within(np.log(np.maximum(f32(a32 * np.float32(1.00002)), np.float32(1e-5))), ref, bound)
    assert not noclamp_ok, "a mel without the 1e-5 clamp passes"


@pytest.mark.parametrize("D", CS.LN_D)
def test_ln_bound(D):
    x, w, b, eps = CS.ln_inputs(D)
    ref, bound = E.ln_rows_ref(x, w, b, eps)
    mean = _sum32(x) / np.float32(D)
    xc = f32(x - mean[:, None])
    inv = np.float32(1) / np.sqrt(_sum32(xc * xc) / np.float32(D) + np.float32(eps))
    assert _within(f32(xc * inv[:, None] * w + b), ref, bound)
    v1 = _sum32(x * x) / np.float32(D) - mean * mean           # one-pass variance: lost at mean 1e3
    with np.errstate(invalid="ignore"):
        inv1 = np.float32(1) / np.sqrt(v1 + np.float32(eps))
    assert not _within(f32(xc * inv1[:, None] * w + b), ref, bound)
    assert not _within(f32(f32(x - f32(mean * np.float32(1.00001))[:, None]) * inv[:, None] * w + b), ref, bound)


def test_egemv_se_rope_bounds():
    for R, Cc in CS.EGEMV:
        W, x, bias = CS.egemv_inputs(R, Cc)
        for act in CS.EGEMV_ACT:
            ref, bound = E.egemv_ref(W, x, bias, act)
            got = E.model_act(act, f32(_sum32(W[None] * x[:, None, :]) + bias))
            assert _within(got, ref, bound)
            assert not _within(E.model_act(act, f32(_sum32(W[None, :, :-1] * x[:, None, :-1]) + bias)), ref, bound)
    for nh, hd in CS.ROPE:
        x, cs, sn = CS.rope_inputs(nh, hd)
        ref, bound = E.rope_ref(x, nh, hd, CS.ROPE_T, cs, sn)
        assert _within(ref.astype(np.float32), ref, bound)
        wrong, _ = E.rope_ref(x, nh, hd, 3 * CS.ROPE_T, np.tile(cs, (3, 1)), np.tile(sn, (3, 1)))   # position = row
        assert np.array_equal(wrong, ref)
        cs15 = np.concatenate([cs, cs[::-1], cs])
        wrong, _ = E.rope_ref(x, nh, hd, 3 * CS.ROPE_T, cs15, np.tile(sn, (3, 1)))
        assert not _within(wrong, ref, bound)


# ------------------------------------------------------------------ k_rvq_enc
@pytest.mark.parametrize("nb,T12,CB", CS.RVQ_EXACT)
def test_rvq_exact_grid(nb, T12, CB):
    lat, psem, pac, cbk, planted = E.rvq_exact_inputs(nb, T12, CB, 0)
    ref = E.rvq_ref(lat, psem, pac, cbk, 1, 16)[0]
    assert len(planted) >= 4 and {j - i for _, _, i, j in planted} >= ({1, 64, 1024, 29} if CB >= 2048 else {1, 64})
    assert np.array_equal(E.rvq_model(lat, psem, pac, cbk, 1, 16), ref)        # fp32, exact on the grid
    last = E.rvq_model(lat, psem, pac, cbk, 1, 16, last_on_ties=True)
    for row, q, i, j in planted:
        assert ref[row, q] == i
        assert q > 0 or last[row, q] == j        # later codebooks: the mutant's chain has already left the reference's
    assert not np.array_equal(last, ref)


@pytest.mark.parametrize("nb,T12,CB,seed", CS.RVQ_RANDOM)
def test_rvq_random_reference_has_no_near_tie(nb, T12, CB, seed):
    """the seed is chosen so that no frame of the float64 reference is within the
    excuse's tolerance: a pass on the device does not rest on the excuse"""
    lat, psem, pac, cbk = E.rvq_random_inputs(nb, T12, CB, seed)
    ref, best, margin, _ = E.rvq_ref(lat, psem, pac, cbk, 1, 16)
    assert np.all(margin > 1e-3 * (1.0 + best)), float(np.min(margin - 1e-3 * (1.0 + best)))
    assert E.check_codes(E.rvq_model(lat, psem, pac, cbk, 1, 16), ref, margin, best) == 0
