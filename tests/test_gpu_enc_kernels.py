"""Every kernel of k_enc.hip on the device through the kernel-level entries
(qtts_hip_econv_case, qtts_hip_enc_op, qtts_hip_enc_func), against the float64
references and bounds of enc_kernel_ref.py on the cases of enc_kernel_cases.py.

Every k_econv case: the rows / kz the library reports are the ones the case
was written for; every output within the bound (the exact-plane instruments:
bit-equal to float64); the inputs are NaN outside what the launch may read and
the outputs and the split-K workspace are prefilled with a sentinel, and
everything outside the written pattern comes back bit-identical.
test_enc_kernel_ref.py checks on the same inputs that the bounds would notice
a wrong kernel."""
import math

import numpy as np
import pytest

import enc_kernel_cases as CS
import enc_kernel_ref as E
import qtts

pytestmark = pytest.mark.gpu

_RATIO = {}


def _dev(a, gpu):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _note(name, ratio):
    _RATIO[name] = max(_RATIO.get(name, 0.0), ratio)
    print(f"err / bound  {name:24s} {ratio:.4f}")


def _within(name, got, ref, bound):
    got = np.asarray(got, np.float64)
    assert np.all(np.isfinite(got)), name
    err = np.abs(got - ref)
    ratio = float(np.max(err / bound)) if err.size else 0.0
    _note(name, ratio)
    assert np.all(err <= bound), (name, ratio, np.argwhere(~(err <= bound))[:4])


def _same(after, before, keep=None):
    a, b = after.view(np.uint32), before.view(np.uint32)
    return np.array_equal(a, b) if keep is None else np.array_equal(a[keep], b[keep])


# ------------------------------------------------------------------ k_econv
@pytest.mark.parametrize("cv", CS.CASES, ids=[cv.id() for cv in CS.CASES])
def test_econv(gpu, cv):
    import torch
    ref = E.reference(cv)
    lo = E.layout(cv, ref[0])
    dev = {k: _dev(lo[k], gpu) for k in ("w", "x", "x2", "y", "bias", "bias2", "vec") if k in lo}
    need = qtts.Kernels.econv_plan(CS.describe(cv, lo, {k: t.data_ptr() for k, t in dev.items()}))["part_elems"]
    part0 = np.full(need + E.PART_TAIL, E.SENTINEL, np.float32)
    part = _dev(part0, gpu)
    desc = CS.describe(cv, lo, {k: t.data_ptr() for k, t in dev.items()}, part.data_ptr(), need)
    ran = qtts.Kernels.econv_case(desc)
    torch.cuda.synchronize()
    assert ran is not None, cv.id()
    assert (ran["rows"], ran["kz"]) == (cv.rows, cv.kz), (ran, cv.id())
    assert ran["part_elems"] == need == (cv.kz * cv.nb * cv.M * cv.nmax if cv.kz > 1 else 0)
    ratio = E.check(cv, lo, dev["y"].cpu().numpy(), ref)
    assert _same(part.cpu().numpy()[need:], part0[need:]), "a write behind the split-K workspace"
    for k in ("w", "x", "x2", "bias", "bias2", "vec"):
        if k in lo:
            assert _same(dev[k].cpu().numpy(), lo[k]), f"the launch wrote to its input {k}"
    _note(("exact " if cv.exact else "") + cv.name + (" split" if cv.kz > 1 else ""), ratio)


def test_econv_own_workspace(gpu):
    """part NULL: the entry allocates what the plan needs (the model's path)"""
    import torch
    cv = CS.CAP[0]
    lo = E.layout(cv, E.reference(cv)[0])
    dev = {k: _dev(lo[k], gpu) for k in ("w", "x", "y", "bias")}
    ran = qtts.Kernels.econv_case(CS.describe(cv, lo, {k: t.data_ptr() for k, t in dev.items()}))
    torch.cuda.synchronize()
    assert (ran["rows"], ran["kz"]) == (cv.rows, cv.kz)
    E.check(cv, lo, dev["y"].cpu().numpy())


# ------------------------------------------------------------------ device functions
def test_device_functions(gpu):
    """erff and expm1f as k_econv calls them, against float64 over the range of
    these tests' arguments, 2^20 points each: within FUNC_ERR_MAX (absolute), so
    the bounds add nothing for them beyond d_in's FUNC_ERR_MAX"""
    import torch
    for fn, name, f64 in ((0, "erff", np.vectorize(math.erf)), (1, "expm1f", np.expm1)):
        lo_, hi_, recorded = E.MEASURED[name]
        v = np.linspace(lo_, hi_, 1 << 20, dtype=np.float64).astype(np.float32)
        out = torch.zeros(v.size, device=gpu)
        qtts.Kernels.enc_func(out, _dev(v, gpu), fn)
        torch.cuda.synchronize()
        m = float(np.max(np.abs(out.cpu().numpy().astype(np.float64) - f64(v.astype(np.float64)))))
        print(f"measured  {name}: largest absolute error {m:.3e} over [{lo_}, {hi_}] (recorded {recorded:.1e})")
        assert m <= E.FUNC_ERR_MAX


# ------------------------------------------------------------------ the small kernels
def _padded(a, pad, fill=np.nan):
    """a [..., L] with `pad` columns of fill behind every row"""
    out = np.full(a.shape[:-1] + (a.shape[-1] + pad,), fill, a.dtype)
    out[..., :a.shape[-1]] = a
    return out


def _ragged_nan(x, lens):
    x = x.copy()
    for b, L in enumerate(lens):
        x[b, ..., L:] = np.nan
    return x


@pytest.mark.parametrize("Cn", CS.STAT_C)
def test_row_mean_asp_stats_asp_pool(gpu, Cn):
    import torch
    x, lg, lens = CS.stats_inputs(Cn)
    nb, Lm = x.shape[0], x.shape[2]
    Ct = Cn + 2                                           # the utterance stride covers two more (NaN) channels
    xs = np.full((nb, Ct, Lm), np.nan, np.float32)
    xs[:, :Cn] = _ragged_nan(x, lens)
    ls = np.full((nb, Ct + 1, Lm), np.nan, np.float32)
    ls[:, :Cn] = _ragged_nan(lg, lens)
    dx, dl, dlen = _dev(xs, gpu), _dev(ls, gpu), _dev(lens, gpu)
    outs = {}
    for name, op, inp, s, width in (("k_row_mean", qtts.EO_ROW_MEAN, (dx, dlen), (Ct * Lm,), Cn),
                                    ("k_asp_stats", qtts.EO_ASP_STATS, (dx, dlen), (Ct * Lm,), 2 * Cn),
                                    ("k_asp_pool", qtts.EO_ASP_POOL, (dx, dl, dlen), (Ct * Lm, (Ct + 1) * Lm), 2 * Cn)):
        o0 = np.full(nb * width + 9, E.SENTINEL, np.float32)
        o = _dev(o0, gpu)
        assert qtts.Kernels.enc_op(op, inp, (o,), (Lm, Cn, nb), s)
        torch.cuda.synchronize()
        got = o.cpu().numpy()
        assert _same(got[nb * width:], o0[nb * width:]), name
        outs[name] = got[:nb * width].reshape(nb, width)
    for b, L in enumerate(lens):
        _within("k_row_mean", outs["k_row_mean"][b], *E.mean_ref(x[b][:, :L]))
        mean, std, b_mean, b_std = E.asp_stats_ref(x[b][:, :L])
        _within("k_asp_stats mean", outs["k_asp_stats"][b, :Cn], mean, b_mean)
        _within("k_asp_stats std", outs["k_asp_stats"][b, Cn:], std, b_std)
        mean, std, b_mean, b_std = E.asp_pool_ref(x[b][:, :L], lg[b][:, :L])
        _within("k_asp_pool mean", outs["k_asp_pool"][b, :Cn], mean, b_mean)
        _within("k_asp_pool std", outs["k_asp_pool"][b, Cn:], std, b_std)


@pytest.mark.parametrize("R,Cc", CS.EGEMV)
def test_egemv(gpu, R, Cc):
    import torch
    W, x, bias = CS.egemv_inputs(R, Cc)
    nb, ldx, ldy = x.shape[0], Cc + 3, R + 2
    dW, dx, db = _dev(W, gpu), _dev(_padded(x, 3), gpu), _dev(bias, gpu)
    for act in CS.EGEMV_ACT:
        for bb in (bias, None):
            y0 = np.full((nb, ldy), E.SENTINEL, np.float32)
            y = _dev(y0, gpu)
            assert qtts.Kernels.enc_op(qtts.EO_EGEMV, (dW, dx, db if bb is not None else None), (y,),
                                       (R, Cc, ldx, act, ldy, nb))
            torch.cuda.synchronize()
            got = y.cpu().numpy()
            assert _same(got[:, R:], y0[:, R:])
            _within(f"k_egemv act {act}", got[:, :R], *E.egemv_ref(W, x, bb, act))


def test_se_apply(gpu):
    import torch
    rng = E._rng("se")
    Cn, lens, Cres = CS.SE["C"], np.array(CS.SE["lens"], np.int32), CS.SE["Cres"]
    nb, ldt = len(lens), int(max(lens))
    h = _ragged_nan(rng.standard_normal((nb, Cn, ldt)).astype(np.float32), lens)
    res = np.full((nb, Cres, ldt), np.nan, np.float32)
    res[:, :Cn] = _ragged_nan(rng.standard_normal((nb, Cn, ldt)).astype(np.float32), lens)
    s = rng.uniform(0, 1, (nb, Cn)).astype(np.float32)
    o0 = np.full((nb, Cn + 1, ldt), E.SENTINEL, np.float32)
    o = _dev(o0, gpu)
    assert qtts.Kernels.enc_op(qtts.EO_SE_APPLY, (_dev(h, gpu), _dev(s, gpu), _dev(res, gpu), _dev(lens, gpu)), (o,),
                               (Cn, ldt, nb), (Cn * ldt, Cres * ldt, (Cn + 1) * ldt))
    torch.cuda.synchronize()
    got = o.cpu().numpy()
    keep = np.ones(o0.shape, bool)
    for b, L in enumerate(lens):
        keep[b, :Cn, :L] = False
        _within("k_se_apply", got[b, :Cn, :L], *E.se_apply_ref(h[b, :, :L], s[b], res[b, :Cn, :L]))
    assert _same(got, o0, keep)


@pytest.mark.parametrize("D", CS.LN_D)
def test_ln_rows(gpu, D):
    import torch
    x, w, b, eps = CS.ln_inputs(D)
    y0 = np.full(x.size + 8, E.SENTINEL, np.float32)
    y = _dev(y0, gpu)
    assert qtts.Kernels.enc_op(qtts.EO_LN_ROWS, (_dev(x, gpu), _dev(w, gpu), _dev(b, gpu)), (y,), (x.shape[0], D),
                               eps=eps)
    torch.cuda.synchronize()
    got = y.cpu().numpy()
    assert _same(got[x.size:], y0[x.size:])
    _within("k_ln_rows", got[:x.size].reshape(x.shape), *E.ln_rows_ref(x, w, b, np.float64(np.float32(eps))))


@pytest.mark.parametrize("nh,hd", CS.ROPE)
def test_rope_bt(gpu, nh, hd):
    import torch
    x, cs, sn = CS.rope_inputs(nh, hd)
    R, ld = x.shape[0], nh * hd + 4
    x0 = _padded(x, 4, E.SENTINEL)
    dx = _dev(x0, gpu)
    assert qtts.Kernels.enc_op(qtts.EO_ROPE_BT, (_dev(cs, gpu), _dev(sn, gpu)), (dx,), (R, ld, nh, hd, CS.ROPE_T))
    torch.cuda.synchronize()
    got = dx.cpu().numpy()
    assert _same(got[:, nh * hd:], x0[:, nh * hd:])
    _within("k_rope_bt", got[:, :nh * hd], *E.rope_ref(x, nh, hd, CS.ROPE_T, cs, sn))


@pytest.mark.parametrize("R,T", [(1, 1), (15, 5), (257, 7)])
def test_rows_bt(gpu, R, T):
    import torch
    rb, pos = (_dev(np.full(R + 3, E.ISENT, np.int32), gpu) for _ in range(2))
    assert qtts.Kernels.enc_op(qtts.EO_ROWS_BT, (), (rb, pos), (R, T))
    torch.cuda.synchronize()
    r = np.arange(R)
    assert np.array_equal(rb.cpu().numpy(), np.concatenate([r // T, [E.ISENT] * 3]))
    assert np.array_equal(pos.cpu().numpy(), np.concatenate([r % T, [E.ISENT] * 3]))


@pytest.mark.parametrize("nf,nm", CS.MEL)
def test_mel(gpu, nf, nm):
    import torch
    spec, fb, flo, fhi, T = CS.mel_inputs(nf, nm)
    nb, ldt = spec.shape[0], spec.shape[2]
    m0 = np.full((nb, nm, ldt), E.SENTINEL, np.float32)
    mel = _dev(m0, gpu)
    assert qtts.Kernels.enc_op(qtts.EO_MEL, (_dev(_ragged_nan(spec, T), gpu), _dev(T, gpu), _dev(fb, gpu),
                                             _dev(flo, gpu), _dev(fhi, gpu)), (mel,), (nf, ldt, nb, nm))
    torch.cuda.synchronize()
    got = mel.cpu().numpy()
    keep = np.ones(m0.shape, bool)
    for b in range(nb):
        keep[b, :, :T[b]] = False
        ref, bound, acc = E.mel_ref(spec[b][:, :T[b]], fb, flo, fhi)
        _within("k_mel", got[b, :, :T[b]], ref, bound)
    assert _same(got, m0, keep)                                          # columns >= T[b] stay untouched


def _run_rvq(gpu, lat, psem, pac, cbk):
    import torch
    nb, hid, T12 = lat.shape
    nv, CB, vq = cbk.shape
    ldc = T12 + 1
    c0 = np.full((nb, ldc, 16), E.ISENT, np.int32)
    codes = _dev(c0, gpu)
    assert qtts.Kernels.enc_op(qtts.EO_RVQ_ENC,
                               (_dev(lat, gpu), _dev(psem.T, gpu), _dev(pac.T, gpu),
                                _dev(np.transpose(cbk, (0, 2, 1)), gpu)), (codes,),
                               (T12, hid, nb * T12, CB, vq, nv, 1, ldc))
    torch.cuda.synchronize()
    got = codes.cpu().numpy()
    assert np.all(got[:, T12:] == E.ISENT)
    return got[:, :T12].reshape(nb * T12, 16)


@pytest.mark.parametrize("nb,T12,CB", CS.RVQ_EXACT)
def test_rvq_exact_grid(gpu, nb, T12, CB):
    """every value of the chain is exact in fp32: all 16 codes of every row
    equal the float64 argmin with the first index on ties, no case excused"""
    lat, psem, pac, cbk, planted = E.rvq_exact_inputs(nb, T12, CB, 0)
    ref = E.rvq_ref(lat, psem, pac, cbk, 1, 16)[0]
    got = _run_rvq(gpu, lat, psem, pac, cbk)
    assert np.array_equal(got, ref), (np.argwhere(got != ref)[:6], planted)


@pytest.mark.parametrize("nb,T12,CB,seed", CS.RVQ_RANDOM)
def test_rvq_random(gpu, nb, T12, CB, seed):
    lat, psem, pac, cbk = E.rvq_random_inputs(nb, T12, CB, seed)
    ref, best, margin, _ = E.rvq_ref(lat, psem, pac, cbk, 1, 16)
    E.check_codes(_run_rvq(gpu, lat, psem, pac, cbk), ref, margin, best)


def test_zz_ratios(gpu):
    """prints the largest err / bound per kernel seen by the cases above (for DESIGN.md)"""
    for k in sorted(_RATIO):
        print(f"err / bound  {k:32s} {_RATIO[k]:.4f}")
