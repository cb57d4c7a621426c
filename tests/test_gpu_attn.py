"""Every attention path against the float64 reference and the absolute bound
of attn_ref.py, at the shipped shapes and at each kernel's own edges.

Paths (k_attn.hip, qtts_attn_dev.h) and the entry that reaches each:
  k_attn_dec     split decode, NH == 2 KV, HD 16..128, S > 16   attn_decode_ex
  k_attn_short   the same heads at S <= 16 (the sub-talker)      attn_decode_ex
  k_attn mode 0  every other head layout                         attn_decode_ex
  k_qk_prep_w    prefill q / k norm + RoPE + cache write         attn_cached prep 1
  k_attn mode 1  cached attention, sliding window                attn_cached prep 0 / 1
  k_attn_o       short attention + O projection by kv head       attn_o
Head sizes that are not a power of two are refused (k_attn's lane groups
cannot serve them), which leaves the k_qk_prep fallback
without a caller.

Inputs: q|k|v rows N(0, 1), norm weights 1 + 0.1 N(0, 1), caches N(0, 1)
rounded to bf16 (the same values serve the fp32 and the bf16 cache).  Random
keys alone let a lost key hide behind a small weight, so every path also runs
with one planted key per row: cache row t* = c q_hat, c = 12 sqrt(HD) /
|q_hat|^2, a score of 12 among N(0, 1) scores, at the split / pass / window
edges; the reference must give it a weight >= 0.5 before the bound is asked.

The sensitivity self-test at the end runs without a GPU: it mutates the
reference (not a kernel) and requires the bound to notice.

Measured err / bound per path on the MI355X: DESIGN.md section 4.
"""
import numpy as np
import pytest

import qtts
from attn_ref import (C_ABS, C_DOT, EPS, attend, norm_rope, rne_bf16, rope_tables, stored_bound, widen, window_lo)

gpu_test = pytest.mark.gpu

# keys per split of k_attn_dec (qtts_attn_keys_per_split at the default lanes per key)
CH = {128: 32, 64: 128, 32: 256, 16: 256}


# ------------------------------------------------------------------ device calls on numpy arrays
def _t(a, dev):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).to(dev)


def _back(t, like):
    a = t.cpu().numpy()
    return a.view(np.uint16) if like.dtype == np.uint16 else a


def dev_decode(qkv, kc, vc, qn, kn, cos, sin, pos, NH, KV, HD, S, skip=None):
    """attn_decode_ex; kc / vc float32 (fp32 cache) or uint16 (bf16 cache).
    Returns (out, kc, vc after the call)."""
    import torch
    dev, rows = torch.device("cuda:0"), len(pos)
    kcd, vcd = _t(kc, dev), _t(vc, dev)
    out = torch.full((rows, NH * HD), float("nan"), dtype=torch.float32, device=dev)
    qtts.Kernels.attn_decode_ex(out, _t(qkv, dev), kcd, vcd, _t(qn, dev), _t(kn, dev), _t(cos[:S], dev), _t(sin[:S], dev),
                                _t(np.asarray(pos, np.int32), dev), NH, KV, HD, S, rows, EPS,
                                1 if kc.dtype == np.uint16 else 0,
                                None if skip is None else _t(np.asarray(skip, np.int32), dev))
    torch.cuda.synchronize()
    return out.cpu().numpy(), _back(kcd, kc), _back(vcd, vc)


def dev_cached(q, kc, vc, qn, kn, cos, sin, row_b, pos, NH, KV, HD, S, win, prep):
    """attn_cached.  Returns (out, q rows, kc, vc after the call)."""
    import torch
    dev, rows = torch.device("cuda:0"), len(pos)
    qd, kcd, vcd = _t(q, dev), _t(kc, dev), _t(vc, dev)
    out = torch.full((rows, NH * HD), float("nan"), dtype=torch.float32, device=dev)
    opt = lambda a: None if a is None else _t(a, dev)
    qtts.Kernels.attn_cached(out, qd, q.shape[1], kcd, vcd, opt(qn), opt(kn), opt(cos), opt(sin),
                             _t(np.asarray(row_b, np.int32), dev), _t(np.asarray(pos, np.int32), dev), NH, KV, HD, S,
                             kc.shape[0], rows, EPS, win, 1 if kc.dtype == np.uint16 else 0, prep)
    torch.cuda.synchronize()
    return out.cpu().numpy(), qd.cpu().numpy(), _back(kcd, kc), _back(vcd, vc)


def dev_attn_o(qkv, kc, vc, qn, kn, cos, sin, pos, wo_bits, R, NH, KV, HD, S):
    """attn_o.  Returns (part [KV, rows, R] or None where not covered, kc, vc)."""
    import torch
    dev, rows = torch.device("cuda:0"), len(pos)
    kcd, vcd = _t(kc, dev), _t(vc, dev)
    part = torch.full((KV, rows, R), float("nan"), dtype=torch.float32, device=dev)
    ran = qtts.Kernels.attn_o(part, _t(qkv, dev), kcd, vcd, _t(qn, dev), _t(kn, dev), _t(cos[:S], dev), _t(sin[:S], dev),
                              _t(np.asarray(pos, np.int32), dev), _t(wo_bits, dev), R, NH, KV, HD, S, rows, EPS)
    torch.cuda.synchronize()
    return (part.cpu().numpy() if ran else None), kcd.cpu().numpy(), vcd.cpu().numpy()


# ------------------------------------------------------------------ inputs
class Inputs:
    """inputs of one shape, shared by every case of it (never modified: a
    planted case works on copies)"""

    def __init__(self, NH, KV, HD, S, slots):
        rng = np.random.default_rng(100000 * S + 1000 * NH + 100 * KV + HD)
        self.NH, self.KV, self.HD, self.S, self.slots = NH, KV, HD, S, slots
        self.W = (NH + 2 * KV) * HD
        self.qkv = rng.standard_normal((max(slots, 32), self.W)).astype(np.float32)
        self.qn = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
        self.kn = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
        self.cos, self.sin = rope_tables(S + 1, HD)   # (+ 1: the self-test's wrong RoPE row)
        self.kbits = rne_bf16(rng.standard_normal((slots, S, KV * HD)).astype(np.float32))
        self.vbits = rne_bf16(rng.standard_normal((slots, S, KV * HD)).astype(np.float32))


_INPUTS = {}


def inputs(NH, KV, HD, S, slots):
    key = (NH, KV, HD, S, slots)
    if key not in _INPUTS:
        _INPUTS[key] = Inputs(*key)
    return _INPUTS[key]


def _heads(row, I):
    """(q [NH, HD], k [KV, HD], v [KV HD]) of a fused row"""
    NH, KV, HD = I.NH, I.KV, I.HD
    return row[:NH * HD].reshape(NH, HD), row[NH * HD:(NH + KV) * HD].reshape(KV, HD), row[(NH + KV) * HD:]


def _mixed(positions, rows):
    """row position lists that together hold every position"""
    n = len(positions)
    return [[positions[(i * rows + r) % n] for r in range(rows)] for i in range((n + rows - 1) // rows)]


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b, msg):
    np.testing.assert_array_equal(_bits(np.ascontiguousarray(a)), _bits(np.ascontiguousarray(b)), err_msg=msg)


def plant_gain(HD):
    """norm weight gain of the planted cases: the token's own key scores
    |q_hat|^2 / sqrt(HD) ~ g^2 sqrt(HD), 12 at every head size"""
    return max(1.0, float(np.sqrt(12.0 / np.sqrt(HD))))


def planted_row(q_hat):
    """c q_hat with c = 12 sqrt(HD) / |q_hat|^2, as bf16 bits"""
    q = np.asarray(q_hat, np.float64)
    return rne_bf16((12.0 * np.sqrt(q.shape[-1]) / (q @ q) * q).astype(np.float32))


_RATIO = {}   # path -> largest err / bound, printed for DESIGN.md


def _note(path, ratio):
    _RATIO[path] = max(_RATIO.get(path, 0.0), float(ratio))


def _report(prefix):
    for k in sorted(_RATIO):
        if k.startswith(prefix):
            print(f"err / bound  {k:52s} {_RATIO[k]:.4f}")


def _assert_bound(path, got, ref, bound, msg):
    err = np.abs(np.asarray(got, np.float64) - ref)
    assert np.isfinite(got).all(), msg
    ratio = float((err / bound).max())
    _note(path, ratio)
    assert ratio <= 1.0, f"{path} {msg}: err / bound {ratio:.3f} (largest err {err.max():.3e})"
    return ratio


# ------------------------------------------------------------------ the decode entry (mode 0: slot = row)
def check_decode(path, I, S, pos, bf16, qkv=None, qn=None, kn=None, kbits=None, vbits=None, skip=None, own=None,
                 plant=None):
    """One attn_decode_ex case on the fp32 cache and, with bf16, on the bf16
    cache holding the same values.  Stored rows, untouched rows, outputs.
    plant: {row: key index} -- the reference weight of that key must be >= 0.5
    for the first query head of every kv head.  skip: per-row flags, with own
    = what the same call without flags returned (the token's own k / v as they
    are stored).  Returns the runs {"fp32": (out, K, V), "bf16": ...}, the
    caches as float32 values."""
    NH, KV, HD, rows = I.NH, I.KV, I.HD, len(pos)
    gph = NH // KV
    qkv = I.qkv[:rows] if qkv is None else qkv
    qn, kn = I.qn if qn is None else qn, I.kn if kn is None else kn
    kb0 = (I.kbits if kbits is None else kbits)[:rows, :S]
    vb0 = (I.vbits if vbits is None else vbits)[:rows, :S]
    skip = [0] * rows if skip is None else skip
    flags = skip if any(skip) else None
    o32, k32, v32 = dev_decode(qkv, widen(kb0), widen(vb0), qn, kn, I.cos, I.sin, pos, NH, KV, HD, S, flags)
    runs = [("fp32", o32, k32, v32)]
    if bf16:
        o16, kb, vb = dev_decode(qkv, kb0, vb0, qn, kn, I.cos, I.sin, pos, NH, KV, HD, S, flags)
        runs.append(("bf16", o16, widen(kb), widen(vb)))
    for r, p in enumerate(pos):
        q, k, v = _heads(qkv[r], I)
        q_hat, _ = norm_rope(q, qn, I.cos[p], I.sin[p])
        k_hat, mag = norm_rope(k, kn, I.cos[p], I.sin[p])
        tag = f"pos {pos} row {r}"
        keep = np.arange(S) != p
        if skip[r]:   # nothing of the slot changes
            _same(k32[r], widen(kb0[r]), "K, skipped " + tag)
            _same(v32[r], widen(vb0[r]), "V, skipped " + tag)
            if bf16:
                _same(kb[r], kb0[r], "K bf16, skipped " + tag)
                _same(vb[r], vb0[r], "V bf16, skipped " + tag)
        else:
            assert (np.abs(k32[r, p] - k_hat.ravel()) <= stored_bound(mag.ravel())).all(), "stored k, " + tag
            _same(v32[r, p], v, "stored v, " + tag)
            _same(k32[r, keep], widen(kb0[r, keep]), "other K rows, " + tag)
            _same(v32[r, keep], widen(vb0[r, keep]), "other V rows, " + tag)
            if bf16:
                _same(kb[r, p], rne_bf16(k32[r, p]), "stored k bf16, " + tag)
                _same(vb[r, p], rne_bf16(v), "stored v bf16, " + tag)
                _same(kb[r, keep], kb0[r, keep], "other K rows bf16, " + tag)
                _same(vb[r, keep], vb0[r, keep], "other V rows bf16, " + tag)
        for name, out, Kc, Vc in runs:
            K, V = Kc[r, :p + 1].astype(np.float64), Vc[r, :p + 1].astype(np.float64)
            if skip[r]:   # the token's own k / v, as the unflagged call stored them
                K[p], V[p] = own[name][1][r, p], own[name][2][r, p]
            ref, bound, P = attend(q_hat, K.reshape(-1, KV, HD), V.reshape(-1, KV, HD))
            if plant is not None and r in plant:
                w = P[::gph, plant[r]]
                assert (w >= 0.5).all(), f"planted key {plant[r]} weighs {w.min():.3f}, {tag}"
            _assert_bound(f"{path} {name}", out[r].reshape(NH, HD), ref, bound, tag)
    return {name: (out, Kc, Vc) for name, out, Kc, Vc in runs}


def planted_decode(path, I, S, p, tstars, bf16):
    """row r attends [0, p] with its dominant key at tstars[r] (p itself: the
    raw k is the raw q halved and kn_w = qn_w, so k_hat = q_hat)"""
    NH, KV, HD, rows = I.NH, I.KV, I.HD, len(tstars)
    gph = NH // KV
    g = np.float32(plant_gain(HD))
    qn = (g * I.qn).astype(np.float32)
    qkv, kbits = I.qkv[:rows].copy(), I.kbits[:rows, :S].copy()
    for r, ts in enumerate(tstars):
        q = _heads(qkv[r], I)[0]
        if ts == p:
            qkv[r, NH * HD:(NH + KV) * HD] = (0.5 * q[::gph]).ravel()
        else:
            q_hat, _ = norm_rope(q, qn, I.cos[p], I.sin[p])
            for kvh in range(KV):
                kbits[r, ts, kvh * HD:(kvh + 1) * HD] = planted_row(q_hat[kvh * gph])
    check_decode(path, I, S, [p] * rows, bf16, qkv=qkv, qn=qn, kn=qn, kbits=kbits, plant=dict(enumerate(tstars)))


# ---- split decode
SPLIT_SHIPPED = [0, 31, 32, 33, 64, 255, 256, 257, 319]   # one split, <= 8 merged, > 8 merged
SPLIT_POS = {128: SPLIT_SHIPPED, 64: [0, 127, 128, 129, 255, 256, 257, 319], 32: [0, 1, 255, 256, 257, 319],
             16: [0, 1, 255, 256, 257, 319]}


@gpu_test
@pytest.mark.parametrize("NH,KV,HD,rows", [(16, 8, 128, 1), (16, 8, 128, 8), (16, 8, 128, 16), (4, 2, 64, 3),
                                           (4, 2, 32, 3), (4, 2, 16, 3)])
def test_split_decode(gpu, NH, KV, HD, rows):
    """k_attn_dec, both cache types: the shipped talker heads at 1, 8 and 16
    lock-step rows with mixed positions, the smaller head sizes at their own
    split edges"""
    I = inputs(NH, KV, HD, 320, 16 if HD == 128 else 5)
    for pos in _mixed(SPLIT_POS[HD], rows):
        check_decode(f"k_attn_dec HD{HD}", I, 320, pos, True)
    _report(f"k_attn_dec HD{HD}")


@gpu_test
@pytest.mark.parametrize("NH,KV,HD", [(16, 8, 128), (4, 2, 64), (4, 2, 32), (4, 2, 16)])
def test_split_decode_planted_key(gpu, NH, KV, HD):
    """the dominant key at 0, on both sides of the first split boundary, at
    p - 1 and at p (the token's own, from LDS), p = 300"""
    I = inputs(NH, KV, HD, 320, 16 if HD == 128 else 5)
    planted_decode(f"k_attn_dec HD{HD} planted", I, 320, 300, [0, CH[HD] - 1, CH[HD], 299, 300], True)
    _report(f"k_attn_dec HD{HD} planted")


# ---- the short kernel
@gpu_test
@pytest.mark.parametrize("NH,KV,HD", [(16, 8, 128), (4, 2, 16)])
@pytest.mark.parametrize("S", [16, 10, 1])
def test_short_decode(gpu, NH, KV, HD, S):
    """k_attn_short (S <= 16), fp32: rows 1 and 16, positions 0, 1, S - 2, S - 1;
    the bf16 cache is refused there"""
    I = inputs(NH, KV, HD, 16, 16)
    positions = sorted({p for p in (0, 1, S - 2, S - 1) if 0 <= p < S})
    for p in positions:
        check_decode(f"k_attn_short HD{HD}", I, S, [p], False)
    check_decode(f"k_attn_short HD{HD}", I, S, [positions[r % len(positions)] for r in range(16)], False)
    with pytest.raises(RuntimeError):
        dev_decode(I.qkv[:1], I.kbits[:1, :S], I.vbits[:1, :S], I.qn, I.kn, I.cos, I.sin, [0], NH, KV, HD, S)
    _report(f"k_attn_short HD{HD} fp32")


@gpu_test
@pytest.mark.parametrize("NH,KV,HD", [(16, 8, 128), (4, 2, 16)])
def test_short_decode_planted_key(gpu, NH, KV, HD):
    I = inputs(NH, KV, HD, 16, 16)
    planted_decode(f"k_attn_short HD{HD} planted", I, 16, 15, [0, 14, 15], False)
    _report(f"k_attn_short HD{HD} planted")


# ---- the generic kernel, mode 0
GENERIC = [(4, 4, 32), (8, 2, 64), (4, 2, 8)]   # no GQA, GQA 4, the smallest head (one lane per key)
GENERIC_POS = [0, 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 319]   # 32 / 64 / 256 keys per pass


@gpu_test
@pytest.mark.parametrize("NH,KV,HD", GENERIC)
def test_generic_decode(gpu, NH, KV, HD):
    """k_attn mode 0 (head layouts the split kernel does not take), both cache types"""
    I = inputs(NH, KV, HD, 320, 5)
    for pos in _mixed(GENERIC_POS, 3):
        check_decode(f"k_attn mode 0 HD{HD}", I, 320, pos, True)
    _report(f"k_attn mode 0 HD{HD}")


@gpu_test
@pytest.mark.parametrize("NH,KV,HD", GENERIC)
def test_generic_decode_planted_key(gpu, NH, KV, HD):
    """the dominant key at 0, on both sides of the first pass boundary (256 /
    (HD / 8) keys per pass), at p - 1 and at p"""
    I = inputs(NH, KV, HD, 320, 5)
    kpp = 256 // (HD // 8)
    planted_decode(f"k_attn mode 0 HD{HD} planted", I, 320, 300, [0, kpp - 1, kpp, 299, 300], True)
    _report(f"k_attn mode 0 HD{HD} planted")


# ---- skip flags
@gpu_test
@pytest.mark.parametrize("NH,KV,HD,S,pos", [(16, 8, 128, 320, [40, 300, 33]), (16, 8, 128, 16, [3, 15, 0]),
                                            (4, 4, 32, 320, [40, 300, 33])])
def test_skip_flags(gpu, NH, KV, HD, S, pos):
    """AttnArgs::skip on the split, the short and the generic kernel: the
    flagged row's slot is bit-unchanged, its output is the attention with the
    token's own k / v all the same, and the other rows do not notice"""
    I = inputs(NH, KV, HD, S, 16 if HD == 128 else 5)
    bf16 = S > 16
    path = "k_attn_short" if S <= 16 else ("k_attn_dec" if NH == 2 * KV else "k_attn mode 0")
    plain = check_decode(f"{path} HD{HD}", I, S, pos, bf16)
    flagged = check_decode(f"{path} HD{HD} skip", I, S, pos, bf16, skip=[0, 1, 0], own=plain)
    for name in plain:
        for r in (0, 2):
            for a, b, what in zip(plain[name], flagged[name], ("output", "K", "V")):
                _same(a[r], b[r], f"{name} {what} of row {r} with another row flagged")
        _same(plain[name][0][1], flagged[name][0][1], f"{name} output of the flagged row")   # (only the store is skipped)
    _report(path)


# ------------------------------------------------------------------ the cached entry
def check_prep(path, I, S, row_b, pos, p0, bf16, q=None, qn=None, kn=None, kbits=None, plant=None):
    """attn_cached prep 1: slots filled below p0[b] (NaN above: a read past a
    row's own keys shows), the rows of this call written by it.  Stored rows
    by the k / v rules, q in place, outputs under the bound."""
    NH, KV, HD, rows = I.NH, I.KV, I.HD, len(pos)
    gph, AD = NH // KV, NH * HD
    q = I.qkv[:rows] if q is None else q
    qn, kn = I.qn if qn is None else qn, I.kn if kn is None else kn
    kb0, vb0 = (I.kbits if kbits is None else kbits)[:, :S].copy(), I.vbits[:, :S].copy()
    for b, n in enumerate(p0):
        kb0[b, n:], vb0[b, n:] = 0x7FC0, 0x7FC0
    f0, g0 = widen(kb0), widen(vb0)
    o32, q32, k32, v32 = dev_cached(q, f0, g0, qn, kn, I.cos, I.sin, row_b, pos, NH, KV, HD, S, 0, 1)
    runs = [("fp32", o32, q32, k32, v32)]
    if bf16:
        o16, q16, kb, vb = dev_cached(q, kb0, vb0, qn, kn, I.cos, I.sin, row_b, pos, NH, KV, HD, S, 0, 1)
        runs.append(("bf16", o16, q16, widen(kb), widen(vb)))
        _same(q16, q32, "q in place: the same under both cache types")
    written = np.zeros((len(p0), S), bool)
    for r, (b, p) in enumerate(zip(row_b, pos)):
        qh, k, v = _heads(q[r], I)
        q_hat, qmag = norm_rope(qh, qn, I.cos[p], I.sin[p])
        k_hat, kmag = norm_rope(k, kn, I.cos[p], I.sin[p])
        tag = f"row {r} (slot {b}, pos {p})"
        written[b, p] = True
        assert (np.abs(q32[r, :AD] - q_hat.ravel()) <= stored_bound(qmag.ravel())).all(), "q in place, " + tag
        _same(q32[r, AD:], q[r, AD:], "k | v of the row, " + tag)
        assert (np.abs(k32[b, p] - k_hat.ravel()) <= stored_bound(kmag.ravel())).all(), "stored k, " + tag
        _same(v32[b, p], v, "stored v, " + tag)
        if bf16:
            _same(kb[b, p], rne_bf16(k32[b, p]), "stored k bf16, " + tag)
            _same(vb[b, p], rne_bf16(v), "stored v bf16, " + tag)
        for name, out, _, Kc, Vc in runs:
            K, V = Kc[b, :p + 1].astype(np.float64), Vc[b, :p + 1].astype(np.float64)
            assert np.isfinite(K).all() and np.isfinite(V).all(), "the test's own rows, " + tag
            ref, bound, P = attend(q_hat, K.reshape(-1, KV, HD), V.reshape(-1, KV, HD))
            if plant is not None and r in plant:
                w = P[::gph, plant[r]]
                assert (w >= 0.5).all(), f"planted key {plant[r]} weighs {w.min():.3f}, {tag}"
            _assert_bound(f"{path} {name}", out[r].reshape(NH, HD), ref, bound, tag)
    keep = ~written
    _same(k32[keep], f0[keep], "other K rows")
    _same(v32[keep], g0[keep], "other V rows")
    if bf16:
        _same(kb[keep], kb0[keep], "other K rows bf16")
        _same(vb[keep], vb0[keep], "other V rows bf16")


P0 = [5, 40]
NEW = [20, 7]


def _interleaved():
    """20 rows of slot 0 from position 5 and 7 of slot 1 from 40, interleaved"""
    row_b, pos = [], []
    for i in range(max(NEW)):
        for b in (0, 1):
            if i < NEW[b]:
                row_b.append(b)
                pos.append(P0[b] + i)
    return row_b, pos


@gpu_test
@pytest.mark.parametrize("NH,KV,HD,bf16", [(16, 8, 128, True), (4, 2, 8, False)])
def test_cached_prep(gpu, NH, KV, HD, bf16):
    """k_qk_prep_w + k_attn mode 1 as the talker prefill issues them (HD 128:
    a lane holds its own rotate-half partner; HD 8: the partner one shuffle away)"""
    I = inputs(NH, KV, HD, 64, 2)
    row_b, pos = _interleaved()
    check_prep(f"k_qk_prep_w + k_attn mode 1 HD{HD}", I, 64, row_b, pos, P0, bf16)
    _report(f"k_qk_prep_w + k_attn mode 1 HD{HD}")


@gpu_test
@pytest.mark.parametrize("NH,KV,HD,bf16", [(16, 8, 128, True), (4, 2, 8, False)])
def test_cached_prep_planted_key(gpu, NH, KV, HD, bf16):
    """dominant keys: slot 0's first new row (pos 5) at key 4 = p - 1, slot
    1's first new row (pos 40) at key 0, both cache rows from before the call;
    slot 0's last row (pos 24) at its own key, written by the call"""
    I = inputs(NH, KV, HD, 64, 2)
    gph = NH // KV
    row_b, pos = _interleaved()
    qn = (np.float32(plant_gain(HD)) * I.qn).astype(np.float32)
    q, kbits = I.qkv[:len(pos)].copy(), I.kbits.copy()
    plant = {}
    for b, p, ts in ((0, 5, 4), (1, 40, 0), (0, 24, 24)):
        r = [i for i in range(len(pos)) if (row_b[i], pos[i]) == (b, p)][0]
        qh = _heads(q[r], I)[0]
        plant[r] = ts
        if ts == p:
            q[r, NH * HD:(NH + KV) * HD] = (0.5 * qh[::gph]).ravel()
        else:
            q_hat, _ = norm_rope(qh, qn, I.cos[p], I.sin[p])
            for kvh in range(KV):
                kbits[b, ts, kvh * HD:(kvh + 1) * HD] = planted_row(q_hat[kvh * gph])
    check_prep(f"k_qk_prep_w + k_attn mode 1 HD{HD} planted", I, 64, row_b, pos, P0, bf16, q=q, qn=qn, kn=qn,
               kbits=kbits, plant=plant)
    _report(f"k_qk_prep_w + k_attn mode 1 HD{HD} planted")


def check_window(path, I, S, row_b, pos, win, q=None, kbits=None, plant=None, outside=None):
    """attn_cached prep 0 (the codec's and the encoder's call): q and the
    caches as they are, keys [max(0, p + 1 - win), p] of slot row_b.  plant:
    {row: key index}; outside: {row: key index just below the window} -- a
    reference that took that key would give it >= 0.5."""
    NH, KV, HD, rows = I.NH, I.KV, I.HD, len(pos)
    gph = NH // KV
    q = I.qkv[:rows, :NH * HD] if q is None else q
    kb = (I.kbits if kbits is None else kbits)[:, :S]
    Kc, Vc = widen(kb), widen(I.vbits[:, :S])
    out, q1, k1, v1 = dev_cached(np.ascontiguousarray(q), Kc, Vc, None, None, None, None, row_b, pos, NH, KV, HD, S, win, 0)
    _same(q1, q, "q untouched")
    _same(k1, Kc, "K cache untouched")
    _same(v1, Vc, "V cache untouched")
    for r, (b, p) in enumerate(zip(row_b, pos)):
        lo = window_lo(p, win)
        tag = f"row {r} (slot {b}, pos {p})"
        K, V = Kc[b, lo:p + 1].reshape(-1, KV, HD), Vc[b, lo:p + 1].reshape(-1, KV, HD)
        ref, bound, P = attend(q[r].reshape(NH, HD), K, V)
        if plant is not None and r in plant:
            w = P[::gph, plant[r] - lo]
            assert (w >= 0.5).all(), f"planted key {plant[r]} weighs {w.min():.3f}, {tag}"
        if outside is not None and r in outside:
            assert outside[r] == lo - 1
            Pm = attend(q[r].reshape(NH, HD), Kc[b, lo - 1:p + 1].reshape(-1, KV, HD), Vc[b, lo - 1:p + 1].reshape(-1, KV, HD))[2]
            assert (Pm[::gph, 0] >= 0.5).all(), f"the key outside the window would weigh {Pm[::gph, 0].min():.3f}, {tag}"
        _assert_bound(path, out[r].reshape(NH, HD), ref, bound, tag)


# (NH, KV, HD, win, S, positions): the codec transformer, the voice-clone encoder, the tiny encoder
WINDOWED = [(16, 16, 64, 72, 160, [0, 70, 71, 72, 73, 150]), (8, 8, 64, 250, 320, [248, 249, 250, 251, 300]),
            (4, 4, 16, 16, 64, [0, 14, 15, 16, 17, 40])]


@gpu_test
@pytest.mark.parametrize("NH,KV,HD,win,S,pos", WINDOWED)
def test_cached_window(gpu, NH, KV, HD, win, S, pos):
    """k_attn mode 1 with the sliding window, positions on both sides of the
    first full window, rows alternating between two slots; then win 0 on the
    same inputs"""
    I = inputs(NH, KV, HD, S, 2)
    row_b = [r % 2 for r in range(len(pos))]
    check_window(f"k_attn mode 1 HD{HD} win {win}", I, S, row_b, pos, win)
    check_window(f"k_attn mode 1 HD{HD} win 0", I, S, row_b, pos, 0)
    _report(f"k_attn mode 1 HD{HD} win")


@gpu_test
@pytest.mark.parametrize("NH,KV,HD,win,S,pos", WINDOWED)
def test_cached_window_planted_key(gpu, NH, KV, HD, win, S, pos):
    """row p = the largest position: the dominant key at the window's first
    key, just outside the window (it must NOT count), at p - 1 and at p; win
    0: at key 0"""
    I = inputs(NH, KV, HD, S, 2)
    p = pos[-1]
    lo = window_lo(p, win)
    assert lo >= 1
    q = I.qkv[:4, :NH * HD]
    for win_, ts, out in ((win, lo, False), (win, lo - 1, True), (win, p - 1, False), (win, p, False), (0, 0, False)):
        kbits = I.kbits.copy()
        for h in range(NH):   # (KV == NH on these paths)
            kbits[1, ts, h * HD:(h + 1) * HD] = planted_row(q[0, h * HD:(h + 1) * HD])
        check_window(f"k_attn mode 1 HD{HD} win {win_} planted", I, S, [1, 0, 1, 0], [p, p, p - 1, 3], win_, q=q, kbits=kbits,
                     plant=None if out else {0: ts}, outside={0: ts} if out else None)
    _report(f"k_attn mode 1 HD{HD} win")


# ------------------------------------------------------------------ attention + O projection
def check_attn_o(path, I, R, pos, S=16, qkv=None, qn=None, kn=None, kbits=None, plant=None):
    NH, KV, HD, rows = I.NH, I.KV, I.HD, len(pos)
    AD = NH * HD
    rng = np.random.default_rng(7 * R + HD)
    wo_bits = rne_bf16((rng.standard_normal((R, AD)) / np.sqrt(AD)).astype(np.float32))
    Wo = widen(wo_bits).astype(np.float64)
    qkv = I.qkv[:rows] if qkv is None else qkv
    qn, kn = I.qn if qn is None else qn, I.kn if kn is None else kn
    kb0, vb0 = (I.kbits if kbits is None else kbits)[:rows, :S], I.vbits[:rows, :S]
    K0, V0 = widen(kb0), widen(vb0)
    part, k1, v1 = dev_attn_o(qkv, K0, V0, qn, kn, I.cos, I.sin, pos, wo_bits, R, NH, KV, HD, S)
    assert part is not None, "covered shape refused"
    for r, p in enumerate(pos):
        q, k, v = _heads(qkv[r], I)
        q_hat, _ = norm_rope(q, qn, I.cos[p], I.sin[p])
        k_hat, mag = norm_rope(k, kn, I.cos[p], I.sin[p])
        tag = f"R {R} pos {pos} row {r}"
        keep = np.arange(S) != p
        assert (np.abs(k1[r, p] - k_hat.ravel()) <= stored_bound(mag.ravel())).all(), "stored k, " + tag
        _same(v1[r, p], v, "stored v, " + tag)
        _same(k1[r, keep], K0[r, keep], "other K rows, " + tag)
        _same(v1[r, keep], V0[r, keep], "other V rows, " + tag)
        att, batt, P = attend(q_hat, k1[r, :p + 1].reshape(-1, KV, HD), v1[r, :p + 1].reshape(-1, KV, HD))
        if plant is not None and r in plant:
            assert (P[::2, plant[r]] >= 0.5).all(), f"planted key {plant[r]} weighs {P[::2, plant[r]].min():.3f}, {tag}"
        for g in range(KV):
            Wg = Wo[:, 2 * HD * g:2 * HD * (g + 1)]
            a, ba = att[2 * g:2 * g + 2].ravel(), batt[2 * g:2 * g + 2].ravel()
            ref = Wg @ a
            bound = C_DOT * (np.abs(Wg) @ np.abs(a)) + np.abs(Wg) @ ba + C_ABS
            _assert_bound(path, part[g, r], ref, bound, f"{tag} kv head {g}")


ATTN_O = [(16, 8, 128, 1024), (4, 2, 16, 64), (4, 2, 16, 100)]   # (R 100: a ragged last row block)


@gpu_test
@pytest.mark.parametrize("NH,KV,HD,R", ATTN_O)
def test_attn_o(gpu, NH, KV, HD, R):
    """k_attn_o: rows 1 and 8, positions 0, 7, 15 of a 16-row cache"""
    I = inputs(NH, KV, HD, 16, 16)
    for p in (0, 7, 15):
        check_attn_o(f"k_attn_o HD{HD}", I, R, [p])
    check_attn_o(f"k_attn_o HD{HD}", I, R, [0, 7, 15, 1, 14, 15, 0, 8])
    _report(f"k_attn_o HD{HD}")


@gpu_test
@pytest.mark.parametrize("NH,KV,HD,R", ATTN_O)
def test_attn_o_planted_key(gpu, NH, KV, HD, R):
    I = inputs(NH, KV, HD, 16, 16)
    gph, p, tstars = 2, 15, [0, 14, 15]
    qn = (np.float32(plant_gain(HD)) * I.qn).astype(np.float32)
    qkv, kbits = I.qkv[:3].copy(), I.kbits[:3].copy()
    for r, ts in enumerate(tstars):
        q = _heads(qkv[r], I)[0]
        if ts == p:
            qkv[r, NH * HD:(NH + KV) * HD] = (0.5 * q[::gph]).ravel()
        else:
            q_hat, _ = norm_rope(q, qn, I.cos[p], I.sin[p])
            for kvh in range(KV):
                kbits[r, ts, kvh * HD:(kvh + 1) * HD] = planted_row(q_hat[kvh * gph])
    check_attn_o(f"k_attn_o HD{HD} planted", I, R, [p] * 3, qkv=qkv, qn=qn, kn=qn, kbits=kbits,
                 plant=dict(enumerate(tstars)))
    _report(f"k_attn_o HD{HD} planted")


@gpu_test
def test_attn_o_reports_shapes_it_does_not_cover(gpu):
    """NH != 2 KV and S = 17 return 1 (nothing launched: the output and the caches keep their bits)"""
    for NH, KV, HD, S in ((4, 4, 16, 16), (8, 2, 16, 16), (4, 2, 16, 17), (4, 2, 8, 16)):
        I = inputs(NH, KV, HD, 32, 2)
        wo_bits = rne_bf16(np.ones((64, NH * HD), np.float32))
        K0, V0 = widen(I.kbits[:2, :S]), widen(I.vbits[:2, :S])
        part, k1, v1 = dev_attn_o(I.qkv[:2], K0, V0, I.qn, I.kn, I.cos, I.sin, [1, 2], wo_bits, 64, NH, KV, HD, S)
        assert part is None, (NH, KV, HD, S)
        _same(k1, K0, "K cache")
        _same(v1, V0, "V cache")


# ------------------------------------------------------------------ head sizes that are not a power of two
@gpu_test
@pytest.mark.parametrize("NH,KV,HD", [(4, 2, 24), (4, 4, 40), (4, 2, 96)])
def test_attention_refuses_head_sizes_that_are_no_power_of_two(gpu, NH, KV, HD):
    """k_attn's lane groups (HD / 8 lanes per key reduced by xor shuffles, 256
    / (HD / 8) keys per pass) are wrong for these (measured before the
    refusal: DESIGN.md section 4), so qtts_attention refuses them, on both
    entries, and nothing is written"""
    I = inputs(NH, KV, HD, 320, 2)
    K0, V0 = widen(I.kbits[:2]), widen(I.vbits[:2])
    with pytest.raises(RuntimeError):
        dev_decode(I.qkv[:2], K0, V0, I.qn, I.kn, I.cos, I.sin, [40, 300], NH, KV, HD, 320)
    for prep in (0, 1):
        q = I.qkv[:2] if prep else np.ascontiguousarray(I.qkv[:2, :NH * HD])
        with pytest.raises(RuntimeError):
            dev_cached(q, K0, V0, I.qn, I.kn, I.cos, I.sin, [0, 1], [40, 300], NH, KV, HD, 320, 0, prep)


@gpu_test
@pytest.mark.parametrize("tag,ov,loads", [("talker_hd48", dict(HD=48, mrope=[12, 6, 6]), False),
                                          ("subtalker_hd48", dict(HDs=48), False),
                                          ("talker_hd64", dict(HD=64, mrope=[16, 8, 8]), True)])
def test_load_refuses_head_sizes_that_are_no_power_of_two(gpu, capfd, tag, ov, loads):
    """qtts_dev_finalize: the tiny model with a 48-wide talker or sub-talker
    head (every width still a multiple of 64) does not load, with the
    head_dim message; the same model with a 64-wide talker head does"""
    import os
    from conftest import MODEL_ROOT
    from synth_model import ensure_model
    md = ensure_model(os.path.join(MODEL_ROOT, "tiny_" + tag), "tiny", seed=0, overrides=ov)
    if loads:
        qtts.QwenTTS(md).close()
        return
    with pytest.raises(RuntimeError):
        qtts.QwenTTS(md)
    assert "unsupported head_dim" in capfd.readouterr().err


# ------------------------------------------------------------------ sensitivity of the bound (no GPU)
def _rate(flags):
    return float(np.mean(flags))


def _flag(mut, ref, bound):
    """per head: does the mutated reference leave the bound"""
    return (np.abs(mut - ref) > bound).any(axis=-1)


# (NH, KV, HD, S, win, positions): the shipped talker, the smallest split head, the generic kernel's smallest
# head, the short kernel, the codec and the tiny encoder windows -- the inputs of the GPU tests above
SENS = [(16, 8, 128, 320, 0, [1, 31, 32, 33, 64, 255, 256, 257, 300, 319]), (4, 2, 16, 320, 0, [1, 2, 5, 31, 32, 33, 64, 255, 256, 257, 300, 319]),
        (4, 2, 8, 320, 0, [1, 2, 5, 31, 32, 33, 64, 255, 256, 257, 300, 319]), (16, 8, 128, 16, 0, [1, 2, 7, 14, 15]),
        (16, 16, 64, 160, 72, [70, 71, 72, 73, 100, 150]), (4, 4, 16, 64, 16, [14, 15, 16, 17, 30, 40])]


@pytest.mark.parametrize("NH,KV,HD,S,win,positions", SENS)
def test_bound_notices_a_wrong_reference(NH, KV, HD, S, win, positions):
    """On the float64 reference alone, one mutation at a time: a key dropped, a
    key counted twice, the scale 1 / sqrt(HD + 1), the RoPE row p + 1 for q,
    the window edge one key off either way.  Each must leave the bound in at
    least 99 % of its (head, key) or (head, position) cases -- what a kernel
    with that defect would do to the GPU assertions above.  (Positions >= 1:
    with one key every softmax weight is 1 and none of the last three
    mutations changes anything.)"""
    slots = {320: 16 if HD == 128 else 5, 16: 16}.get(S, 2)
    I = inputs(NH, KV, HD, S, slots)
    gph = NH // KV
    flags = {k: [] for k in ("drop", "twice", "scale", "rope", "edge")}
    for i, p in enumerate(positions):
        r = i % min(slots, 3)
        lo = window_lo(p, win)
        q, qn = _heads(I.qkv[r], I)[0], I.qn
        q_hat = norm_rope(q, qn, I.cos[p], I.sin[p])[0]
        Kc, Vc = widen(I.kbits[r]).reshape(S, KV, HD).astype(np.float64), widen(I.vbits[r]).reshape(S, KV, HD).astype(np.float64)
        K, V = Kc[lo:p + 1], Vc[lo:p + 1]
        ref, bound, P = attend(q_hat, K, V)
        for h in range(NH):   # every key of the window, in closed form: drop (out - p v) / (1 - p), twice (out + p v) / (1 + p)
            pw, v = P[h][:, None], V[:, h // gph]
            flags["drop"] += list((np.abs(pw * (ref[h] - v) / (1 - pw)) > bound[h]).any(axis=1))
            flags["twice"] += list((np.abs(pw * (v - ref[h]) / (1 + pw)) > bound[h]).any(axis=1))
        t = (len(K) - 1) // 2   # (the closed forms against the plain restatement, one key)
        np.testing.assert_allclose(attend(q_hat, np.delete(K, t, 0), np.delete(V, t, 0))[0],
                                   (ref - P[:, t, None] * V[t].repeat(gph, 0)) / (1 - P[:, t, None]), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(attend(q_hat, K, V, dup=t)[0],
                                   (ref + P[:, t, None] * V[t].repeat(gph, 0)) / (1 + P[:, t, None]), rtol=1e-9, atol=1e-12)
        flags["scale"] += list(_flag(attend(q_hat, K, V, scale=1.0 / np.sqrt(HD + 1))[0], ref, bound))
        flags["rope"] += list(_flag(attend(norm_rope(q, qn, I.cos[p + 1], I.sin[p + 1])[0], K, V)[0], ref, bound))
        if win:
            flags["edge"] += list(_flag(attend(q_hat, Kc[lo + 1:p + 1], Vc[lo + 1:p + 1])[0], ref, bound))
            if lo >= 1:
                flags["edge"] += list(_flag(attend(q_hat, Kc[lo - 1:p + 1], Vc[lo - 1:p + 1])[0], ref, bound))
    for name, f in flags.items():
        if f:
            print(f"NH={NH} KV={KV} HD={HD} S={S} win={win}: {name} leaves the bound in {100 * _rate(f):.2f} % of {len(f)} cases")
            assert _rate(f) >= 0.99, (name, _rate(f), len(f))


def test_planted_row_scores_twelve():
    """the planted key's score is 12 to bf16 rounding, whatever the head size"""
    rng = np.random.default_rng(5)
    for HD in (8, 16, 64, 128):
        q = rng.standard_normal(HD)
        s = widen(planted_row(q)).astype(np.float64) @ q / np.sqrt(HD)
        assert abs(s - 12.0) < 0.05, (HD, s)
        assert plant_gain(HD) ** 2 * np.sqrt(HD) >= 12.0 - 1e-9
