"""The sub-talker's positions 0 and 1 as one two-row pass at batch 1
(k_stpair.hip, QTTS_HIP_ST_PAIR): the pair GEMV and the pair attention + O
against the single-row kernels they replace, bit for bit, and the model-level
path against the oracle.

Kernel level: each output row of a pair launch must equal the single-row
launch's row exactly (same arithmetic in the same order), and is also held to
the float64 bars of the single-row tests: the GEMV bar of test_gpu_kernels.py
(2e-6 * sum|w x| + 1e-6; through the SwiGLU epilogue as that file carries it)
and the attention bound of attn_ref.py.  Model level: small models whose
sub-talker shapes take k_gemvw (Hs 1024, Is 1024, HDs 128), with and without
the input projection; qtts_hip_st_pair_passes() proves which path ran.
"""
import numpy as np
import pytest

import qtts
from attn_ref import C_ABS, C_DOT, EPS, attend, norm_rope, rne_bf16, stored_bound, widen
from conftest import golden, model_dir
from oracle_py import DEFAULT, GREEDY, Oracle
from qtts_io import f32_to_bf16, lookup_ids
from synth_model import prompt_ids
from test_gpu_attn import _heads, _same, dev_attn_o, inputs, plant_gain
from test_oracle_golden import RUNS

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(777.25)


def T(a, dev, dtype=None):
    import torch
    a = np.ascontiguousarray(a)
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a)
    if dtype is not None and t.dtype != dtype:
        t = t.view(dtype)
    return t.to(dev)


def bf16_f64(A):
    return (A.astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def pair_passes():
    return int(qtts.lib().qtts_hip_st_pair_passes())


def audio_close(a, ref):
    assert a is not None and a.shape == ref.shape, (None if a is None else a.shape, ref.shape)
    mse = float(np.mean((a.astype(np.float64) - ref) ** 2)) if len(ref) else 0.0
    assert mse < 1e-4, mse
    if len(ref):
        assert np.abs(a - ref).max() < 1e-4, np.abs(a - ref).max()


# ------------------------------------------------------------------ 1. pair GEMV
def run_rows(dev, A, x, w, epi, part, y0, nrows):
    """qtts_hip_resident_matvec_rows_bf16 on nrows rows; returns (out, x_new)"""
    import torch
    R, Cc = A.shape
    out = T(y0.copy(), dev)
    xnew = torch.full((nrows, Cc), float("nan"), dtype=torch.float32, device=dev) if part is not None else None
    ran = qtts.Kernels.resident_matvec_rows_bf16(out, T(A, dev, torch.int16), T(x, dev), None if w is None else T(w, dev),
                                                 1e-6, R, Cc, epi, None if part is None else T(part, dev), xnew, nrows)
    torch.cuda.synchronize()
    assert ran, "covered shape refused"
    return out.cpu().numpy(), None if xnew is None else xnew.cpu().numpy()


# (R, C, epilogue, norm, partials): the smallest shapes k_gemvw takes --
# STORE + norm and RESID at 1024 x 1024, SwiGLU + norm + 8 partials at
# 2048 x 1024, the down shape 1024 x 3072 (three float4 of x per thread)
PAIR_GEMV = [(1024, 1024, 0, True, 0), (1024, 1024, 3, False, 0), (2048, 1024, 4, True, 8), (1024, 3072, 3, False, 0)]


@pytest.mark.parametrize("R,Cc,epi,norm,npart", PAIR_GEMV)
def test_pair_gemv_equals_two_single_row_launches(gpu, R, Cc, epi, norm, npart):
    rng = np.random.default_rng(11 * R + 3 * Cc + epi)
    A = f32_to_bf16((rng.standard_normal((R, Cc)) / np.sqrt(Cc)).astype(np.float32))
    x = (rng.standard_normal((2, Cc)) * 2).astype(np.float32)   # two different rows
    w = (1 + 0.1 * rng.standard_normal(Cc)).astype(np.float32) if norm else None
    part = (rng.standard_normal((npart, 2, Cc)) * 0.5).astype(np.float32) if npart else None
    nout = R // 2 if epi == 4 else R
    y0 = rng.standard_normal((2, nout)).astype(np.float32) if epi == 3 else np.zeros((2, nout), np.float32)
    got, xnew = run_rows(gpu, A, x, w, epi, part, y0, 2)
    for b in range(2):
        one, xone = run_rows(gpu, A, x[b:b + 1], w, epi, None if part is None else part[:, b:b + 1], y0[b:b + 1], 1)
        np.testing.assert_array_equal(got[b].view(np.uint32), one[0].view(np.uint32), err_msg=f"row {b}")
        if part is not None:
            np.testing.assert_array_equal(xnew[b].view(np.uint32), xone[0].view(np.uint32), err_msg=f"x_new row {b}")
        if part is None:   # and the existing single-row entry
            import torch
            out = T(y0[b].copy(), gpu)
            qtts.Kernels.resident_matvec_bf16(out, T(A, gpu, torch.int16), T(x[b:b + 1], gpu),
                                              None if w is None else T(w, gpu), 1e-6, R, Cc, epi)
            torch.cuda.synchronize()
            np.testing.assert_array_equal(got[b].view(np.uint32), out.cpu().numpy().view(np.uint32),
                                          err_msg=f"row {b} vs qtts_hip_resident_matvec_bf16")
    # each row against float64: |err| <= 2e-6 * sum|w x| + 1e-6
    xs = x.astype(np.float64)
    if part is not None:
        xs = xs + part.astype(np.float64).sum(0)
        assert np.abs(xnew - xs).max() <= 1e-5
    xn = xs / np.sqrt((xs ** 2).mean(1, keepdims=True) + 1e-6) * w if norm else xs
    Af = bf16_f64(A)
    acc = xn @ Af.T
    bound = 2e-6 * (np.abs(xn) @ np.abs(Af).T) + 1e-6
    if epi == 0:
        ref = acc
    elif epi == 3:
        ref = y0 + acc
    else:   # SwiGLU over gate|up quads: rows 8q..8q+3 gate, 8q+4..8q+7 up (the bar carried through the epilogue)
        q, bq = acc.reshape(2, -1, 2, 4), bound.reshape(2, -1, 2, 4)
        g, u = q[:, :, 0, :].reshape(2, -1), q[:, :, 1, :].reshape(2, -1)
        ref = g / (1 + np.exp(-g)) * u
        bound = (bq[:, :, 0, :].reshape(2, -1) + bq[:, :, 1, :].reshape(2, -1)) * (np.abs(u) + np.abs(g) + 1)
    err = np.abs(got - ref)
    print(f"pair GEMV {R}x{Cc} epi {epi}: largest err / bound {float((err / bound).max()):.4f}")
    assert np.all(err <= bound), float((err / bound).max())


def test_pair_gemv_reports_shapes_it_does_not_cover(gpu):
    """shapes outside the pair kernel's list return 1 and leave the output alone"""
    import torch
    for R, Cc in ((96, 64), (1024, 2048), (3072, 1024)):
        A = np.zeros((R, Cc), np.uint16)
        out = torch.full((2, R), 3.0, dtype=torch.float32, device=gpu)
        ran = qtts.Kernels.resident_matvec_rows_bf16(out, T(A, gpu, torch.int16), T(np.ones((2, Cc), np.float32), gpu),
                                                     None, 1e-6, R, Cc, 0, None, None, 2)
        torch.cuda.synchronize()
        assert not ran and float(out.min()) == 3.0, (R, Cc)


# ------------------------------------------------------------------ 2. pair attention + O
def dev_attn_o_pair(qkv, kc, vc, qn, kn, cos, sin, wo_bits, R, NH, KV, HD, S, skip=None):
    """attn_o_pair on one slot's caches [S, KV HD].  Returns (part [KV, 2, R] or None, kc, vc after)."""
    import torch
    dev = torch.device("cuda:0")
    kcd, vcd = T(kc, dev), T(vc, dev)
    part = torch.full((KV, 2, R), float("nan"), dtype=torch.float32, device=dev)
    ran = qtts.Kernels.attn_o_pair(part, T(qkv, dev), kcd, vcd, T(qn, dev), T(kn, dev), T(cos[:S], dev), T(sin[:S], dev),
                                   T(wo_bits, dev, torch.int16), R, NH, KV, HD, S, EPS,
                                   None if skip is None else T(np.asarray(skip, np.int32), dev))
    torch.cuda.synchronize()
    return (part.cpu().numpy() if ran else None), kcd.cpu().numpy(), vcd.cpu().numpy()


def _wo(R, AD, HD):
    rng = np.random.default_rng(7 * R + HD)
    return rne_bf16((rng.standard_normal((R, AD)) / np.sqrt(AD)).astype(np.float32))


def check_pair(I, R, S, qkv, qn, kn, plant=False):
    """pair launch == qtts_hip_attn_o for row 0 at position 0, then row 1 at
    position 1, on the same caches; + the float64 bound per row"""
    NH, KV, HD = I.NH, I.KV, I.HD
    wo_bits = _wo(R, NH * HD, HD)
    Wo = widen(wo_bits).astype(np.float64)
    K0 = np.full((S, KV * HD), SENTINEL, np.float32)
    V0 = np.full((S, KV * HD), SENTINEL, np.float32)
    part, k2, v2 = dev_attn_o_pair(qkv, K0, V0, qn, kn, I.cos, I.sin, wo_bits, R, NH, KV, HD, S)
    assert part is not None, "covered shape refused"
    # the single-row kernel, one position after the other on one slot's caches
    pa, k1, v1 = dev_attn_o(qkv[0:1], K0[None], V0[None], qn, kn, I.cos, I.sin, [0], wo_bits, R, NH, KV, HD, S)
    pb, k1, v1 = dev_attn_o(qkv[1:2], k1, v1, qn, kn, I.cos, I.sin, [1], wo_bits, R, NH, KV, HD, S)
    _same(part[:, 0], pa[:, 0], "partials, row 0")
    _same(part[:, 1], pb[:, 0], "partials, row 1")
    _same(k2[:2], k1[0, :2], "K cache rows 0 and 1")
    _same(v2[:2], v1[0, :2], "V cache rows 0 and 1")
    _same(k2[2:], K0[2:], "other K rows")
    _same(v2[2:], V0[2:], "other V rows")
    worst = 0.0
    for r in range(2):
        q, k, v = _heads(qkv[r], I)
        q_hat, _ = norm_rope(q, qn, I.cos[r], I.sin[r])
        k_hat, mag = norm_rope(k, kn, I.cos[r], I.sin[r])
        assert (np.abs(k2[r] - k_hat.ravel()) <= stored_bound(mag.ravel())).all(), f"stored k, row {r}"
        _same(v2[r], v, f"stored v, row {r}")
        att, batt, P = attend(q_hat, k2[:r + 1].reshape(-1, KV, HD), v2[:r + 1].reshape(-1, KV, HD))
        if plant and r == 1:
            assert (P[::2, 0] >= 0.5).all(), f"planted key 0 weighs {P[::2, 0].min():.3f}"
        for g in range(KV):
            Wg = Wo[:, 2 * HD * g:2 * HD * (g + 1)]
            a, ba = att[2 * g:2 * g + 2].ravel(), batt[2 * g:2 * g + 2].ravel()
            ref = Wg @ a
            bound = C_DOT * (np.abs(Wg) @ np.abs(a)) + np.abs(Wg) @ ba + C_ABS
            err = np.abs(part[g, r].astype(np.float64) - ref)
            assert np.isfinite(part[g, r]).all()
            worst = max(worst, float((err / bound).max()))
            assert (err <= bound).all(), f"row {r} kv head {g}: err / bound {float((err / bound).max()):.3f}"
    print(f"k_attn_o2 HD{HD}{' planted' if plant else ''}: largest err / bound {worst:.4f}")
    return part


PAIR_ATTN = [(4, 2, 128, 1024), (4, 2, 16, 64)]


@pytest.mark.parametrize("NH,KV,HD,R", PAIR_ATTN)
def test_pair_attn_o_equals_two_single_row_launches(gpu, NH, KV, HD, R):
    I = inputs(NH, KV, HD, 16, 16)
    check_pair(I, R, 16, I.qkv[:2], I.qn, I.kn)
    check_pair(I, R, 2, I.qkv[2:4], I.qn, I.kn)   # the smallest cache the pair takes


@pytest.mark.parametrize("NH,KV,HD,R", PAIR_ATTN)
def test_pair_attn_o_planted_key_0(gpu, NH, KV, HD, R):
    """row 0's k aligned with row 1's q: key 0 (taken from the launch's own
    staging, not from the cache) carries most of row 1's weight.  A pair
    kernel that ignored key 0 fails the float64 bound here."""
    I = inputs(NH, KV, HD, 16, 16)
    qn = (np.float32(plant_gain(HD)) * I.qn).astype(np.float32)
    qkv = I.qkv[:2].copy()
    q1_hat, _ = norm_rope(_heads(qkv[1], I)[0], qn, I.cos[1], I.sin[1])
    # position 0 leaves k unrotated: k0_hat = k0 / rms(k0) * kn, so k0 = q1_hat / kn puts k0_hat along q1_hat
    qkv[0, NH * HD:(NH + KV) * HD] = (q1_hat[::2] / qn.astype(np.float64)).astype(np.float32).ravel()
    part = check_pair(I, R, 16, qkv, qn, qn, plant=True)
    # the sensitivity this case exists for: row 1's partials without key 0 are outside the bound
    q, k, v = _heads(qkv[1], I)
    k_hat, _ = norm_rope(k, qn, I.cos[1], I.sin[1])
    att1, _, _ = attend(q1_hat, k_hat.reshape(1, KV, HD), np.asarray(v, np.float64).reshape(1, KV, HD))
    Wo = widen(_wo(R, NH * HD, HD)).astype(np.float64)
    miss = np.concatenate([Wo[:, 2 * HD * g:2 * HD * (g + 1)] @ att1[2 * g:2 * g + 2].ravel() for g in range(KV)])
    assert np.abs(miss - part[:, 1].ravel()).max() > 1e-2


def test_pair_attn_o_skip_and_uncovered(gpu):
    """skip[0] keeps both rows out of the cache (partials unchanged); NH != 2 KV,
    a one-row cache and HD 8 return 1 with nothing written"""
    I = inputs(4, 2, 16, 16, 16)
    wo_bits = _wo(64, 64, 16)
    K0 = np.full((16, 32), SENTINEL, np.float32)
    p0, _, _ = dev_attn_o_pair(I.qkv[:2], K0, K0, I.qn, I.kn, I.cos, I.sin, wo_bits, 64, 4, 2, 16, 16)
    p1, k1, v1 = dev_attn_o_pair(I.qkv[:2], K0, K0, I.qn, I.kn, I.cos, I.sin, wo_bits, 64, 4, 2, 16, 16, skip=[1])
    _same(p0, p1, "partials with the skip flag")
    _same(k1, K0, "K cache, skipped")
    _same(v1, K0, "V cache, skipped")
    for NH, KV, HD, S in ((4, 4, 16, 16), (4, 2, 16, 1), (4, 2, 8, 16)):
        J = inputs(NH, KV, HD, 32, 2)
        Kc = np.full((S, KV * HD), SENTINEL, np.float32)
        part, k2, v2 = dev_attn_o_pair(J.qkv[:2], Kc, Kc, J.qn, J.kn, J.cos, J.sin,
                                       rne_bf16(np.ones((64, NH * HD), np.float32)), 64, NH, KV, HD, S)
        assert part is None, (NH, KV, HD, S)
        _same(k2, Kc, "K cache")
        _same(v2, Kc, "V cache")


# ------------------------------------------------------------------ 3. model level
PAIR_MODELS = {"tiny": dict(Hs=1024, Is=1024, HDs=128), "tiny_eq": dict(H=1024, Hs=1024, Is=1024, HDs=128)}


class _Ref:
    """the oracle's results for one model, computed once and shared"""

    def __init__(self, preset):
        self.md = model_dir(preset, **PAIR_MODELS[preset])
        self.ids = prompt_ids("short")
        o = Oracle(self.md)
        try:
            self.H = o.cfg["H"]
            self.hidden = (np.random.default_rng(5).standard_normal(self.H) * 0.5).astype(np.float32)
            self.st_greedy = o.subtalker(self.hidden, 5, top_k=1, top_p=1.0, temp=1.0, seed=42)
            self.st_sampled = o.subtalker(self.hidden, 5, top_k=50, top_p=1.0, temp=0.9, seed=42)
            s, l = lookup_ids(o.cfg, "aiden", "english")
            self.runs = {}
            for name, pp in (("greedy", GREEDY), ("default", DEFAULT)):
                codes, _ = o.generate_codes(self.ids, s, l, max_tokens=4096, fixed=6, seed=42, **pp)
                self.runs[name] = (pp, codes, o.codec_decode(codes))
        finally:
            o.close()


_REFS = {}


def ref_of(preset):
    if preset not in _REFS:
        _REFS[preset] = _Ref(preset)
    return _REFS[preset]


def _subtalker_codes(m, hidden):
    R = {}
    m.set_params(**{"st_top_k": 1, "st_temperature": 1.0, "st_top_p": 1.0})
    R["greedy"] = m.subtalker(hidden, 5)
    m.set_params(seed=42, st_top_k=50, st_temperature=0.9, st_top_p=1.0)
    R["sampled"] = m.subtalker(hidden, 5)
    return R


@pytest.mark.parametrize("preset", sorted(PAIR_MODELS))
def test_model_pair_path_vs_oracle(gpu, monkeypatch, preset):
    ref = ref_of(preset)
    codes = {}
    for sw in ("1", "0"):
        monkeypatch.setenv("QTTS_HIP_ST_PAIR", sw)
        m = qtts.QwenTTS(ref.md)
        try:
            n0 = pair_passes()
            codes[sw] = _subtalker_codes(m, ref.hidden)
            for name, (pp, want, audio) in ref.runs.items():
                m.set_params(max_tokens=4096, fixed=6, seed=42, **pp)
                a = m.generate(ref.ids, "aiden", "english")
                np.testing.assert_array_equal(m.last_codes(), want, err_msg=f"{preset} {name} switch {sw}")
                audio_close(a, audio)
            rose = pair_passes() - n0
            assert (rose > 0) if sw == "1" else (rose == 0), (sw, rose)
            if sw == "1":   # stream = non-stream on the pair path
                pp, want, audio = ref.runs["greedy"]
                m.set_params(max_tokens=4096, fixed=6, seed=42, **pp)
                full = m.generate(ref.ids, "aiden", "english")
                s = m.generate_stream(ref.ids, "aiden", "english", chunk_frames=4)
                np.testing.assert_array_equal(m.last_codes(), want)
                assert s.shape == full.shape and np.abs(s - full).max() < 1e-5
        finally:
            m.close()
    for k, want in (("greedy", ref.st_greedy), ("sampled", ref.st_sampled)):
        np.testing.assert_array_equal(codes["1"][k], codes["0"][k], err_msg=f"{preset} sub-talker {k}: switch on vs off")
        np.testing.assert_array_equal(codes["1"][k], want, err_msg=f"{preset} sub-talker {k} vs the oracle")


# ------------------------------------------------------------------ 4. gate
@pytest.mark.parametrize("env", [{}, {"QTTS_HIP_ATTN_O": "0"}])
def test_pair_path_gate(gpu, tiny_dir, monkeypatch, env):
    """plain tiny (Hs 64: k_gemv1 shapes) and QTTS_HIP_ATTN_O=0 keep the 16-pass
    chain (counter unchanged) and still match their goldens"""
    E = golden("e2e_tiny.npz")
    md = tiny_dir if not env else model_dir("tiny", **PAIR_MODELS["tiny"])
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    m = qtts.QwenTTS(md)
    try:
        n0 = pair_passes()
        if not env:
            for name in ("greedy", "sampled"):
                fx, pp, fixed, mx, seed = RUNS[name]
                m.set_params(max_tokens=mx, fixed=fixed, seed=seed, **pp)
                a = m.generate(prompt_ids("short"), "aiden", "english")
                np.testing.assert_array_equal(m.last_codes(), E[f"{name}_codes"])
                audio_close(a, E[f"{name}_audio"])
        else:   # the k_gemvw-shaped model with the fused attention + O off: against the oracle's runs
            ref = ref_of("tiny")
            for name, (pp, want, audio) in ref.runs.items():
                m.set_params(max_tokens=4096, fixed=6, seed=42, **pp)
                a = m.generate(ref.ids, "aiden", "english")
                np.testing.assert_array_equal(m.last_codes(), want)
                audio_close(a, audio)
        assert pair_passes() == n0, "the pair path ran where it must not"
    finally:
        m.close()
