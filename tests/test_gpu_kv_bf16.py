"""The optional bf16 talker KV cache (QwenTTS.set_kv_cache("bf16"),
QTTS_HIP_KV=bf16, --kv-cache bf16).

Contract under test: every K row (after k-norm and RoPE) and V row of the
talker cache is stored as RNE(bf16) of the fp32 value the fp32 cache holds;
scores, softmax, P.V and the split merge are the fp32 kernels' arithmetic on
the widened values; a token's own k / v enter its attention as the rounded
values.  bf16 mode is outside the bit-exact-against-the-reference bar by
construction, so the model-level checks compare the GPU with itself.

Kernel level (Kernels.attn_decode): the test fills the caches itself with
bf16-representable values (bit patterns for dtype 1, the same values widened
for dtype 0), so every stored value is known exactly.

Measured on the MI355X (max |error| against the float64 reference over every
position / row case of a shape; e32 = the fp32-cache kernel, the yardstick):
see DESIGN.md section 4, "bf16 talker KV cache".
"""
import numpy as np
import pytest

from conftest import manifest, model_dir
from oracle_py import DEFAULT, GREEDY
from synth_model import prompt_ids

import qtts
from attn_ref import EPS, rne_bf16, widen   # (the shared attention test helpers)
from attn_ref import rope_tables as _rope

pytestmark = pytest.mark.gpu


def test_rne_helper_rounds_ties_to_even():
    x = np.array([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0xBF808000], np.uint32).view(np.float32)
    np.testing.assert_array_equal(rne_bf16(x), np.array([0x3F80, 0x3F82, 0x3F81, 0x3F80, 0xBF80], np.uint16))
    np.testing.assert_array_equal(widen(rne_bf16(x)).view(np.uint32) & 0xFFFF, 0)


# ------------------------------------------------------------------ kernel level
S_BIG, S_SMALL = 320, 40
# (NH, KV, HD, S): the split kernel at every head size it has (HD 128: 32 keys
# per split at the default 8 lanes per key; HD 64: 128; HD 32 / 16: 256), the
# generic kernel (NH != 2 KV; HD 8), and a second capacity
SHAPES = [(4, 2, 128, S_BIG), (4, 2, 64, S_BIG), (4, 2, 32, S_BIG), (4, 2, 16, S_BIG), (4, 4, 32, S_BIG),
          (4, 2, 8, S_BIG), (4, 2, 128, S_SMALL)]
# one split, the 32- / 128- / 256-key split boundaries on both sides, more than
# 8 splits of 32, and the last position of the S = 320 cache
POSITIONS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 300, 319]


class Case:
    """inputs of one shape, shared by every position / row case (never modified)"""

    def __init__(self, NH, KV, HD, rows_max=3):
        rng = np.random.default_rng(1000 * NH + 100 * KV + HD)
        self.NH, self.KV, self.HD = NH, KV, HD
        W = (NH + 2 * KV) * HD
        self.qkv = rng.standard_normal((rows_max, W)).astype(np.float32)
        self.qn = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
        self.kn = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
        self.cos, self.sin = _rope(S_BIG, HD)
        # bf16-representable cache contents (K rows at the scale a normalised,
        # rotated k has; V rows at the scale of the raw projections)
        self.kbits = rne_bf16(rng.standard_normal((rows_max, S_BIG, KV * HD)).astype(np.float32))
        self.vbits = rne_bf16(rng.standard_normal((rows_max, S_BIG, KV * HD)).astype(np.float32))


_CASES = {}


def _case(NH, KV, HD):
    key = (NH, KV, HD)
    if key not in _CASES:
        _CASES[key] = Case(NH, KV, HD)
    return _CASES[key]


def _run(c, S, pos, dtype):
    """one attn_decode call: (out [rows, NH HD], K cache, V cache after the call
    as fp32 values, raw bf16 bits or None)"""
    import torch
    rows = len(pos)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    kb, vb = c.kbits[:rows, :S], c.vbits[:rows, :S]
    if dtype == 1:
        kc, vc = t(kb.view(np.int16)), t(vb.view(np.int16))
    else:
        kc, vc = t(widen(kb)), t(widen(vb))
    out = torch.full((rows, c.NH * c.HD), float("nan"), dtype=torch.float32, device=dev)
    qtts.Kernels.attn_decode(out, t(c.qkv[:rows]), kc, vc, t(c.qn), t(c.kn), t(c.cos[:S]), t(c.sin[:S]),
                             t(np.asarray(pos, np.int32)), c.NH, c.KV, c.HD, S, rows, EPS, dtype)
    torch.cuda.synchronize()
    if dtype == 1:
        kbits, vbits = kc.cpu().numpy().view(np.uint16), vc.cpu().numpy().view(np.uint16)
        return out.cpu().numpy(), widen(kbits), widen(vbits), (kbits, vbits)
    return out.cpu().numpy(), kc.cpu().numpy(), vc.cpu().numpy(), None


def _reference(c, pos, kcache, vcache):
    """float64 attention over the stored values (the current token's row as
    the GPU stored it); q normalised and rotated in float64"""
    NH, KV, HD = c.NH, c.KV, c.HD
    half, gph = HD // 2, NH // KV
    out = np.zeros((len(pos), NH * HD))
    for r, p in enumerate(pos):
        cs, sn = c.cos[p].astype(np.float64), c.sin[p].astype(np.float64)
        for h in range(NH):
            x = c.qkv[r, h * HD:(h + 1) * HD].astype(np.float64)
            x = x / np.sqrt(np.mean(x * x) + EPS) * c.qn.astype(np.float64)
            q = np.concatenate([x[:half] * cs[:half] - x[half:] * sn[:half], x[half:] * cs[half:] + x[:half] * sn[half:]])
            kv = h // gph
            K = kcache[r, :p + 1, kv * HD:(kv + 1) * HD].astype(np.float64)
            V = vcache[r, :p + 1, kv * HD:(kv + 1) * HD].astype(np.float64)
            s = K @ q / np.sqrt(HD)
            w = np.exp(s - s.max())
            out[r, h * HD:(h + 1) * HD] = (w / w.sum()) @ V
    return out


def _pos_cases(S):
    ps = [p for p in POSITIONS if p < S] + ([S - 1] if S - 1 not in POSITIONS else [])
    n = len(ps)
    return [[p] for p in ps] + [[ps[i], ps[(i + 5) % n], ps[(i + 11) % n]] for i in range(n)]


_ERRS = {}   # shape -> (e32, e16), printed for DESIGN.md


@pytest.mark.parametrize("NH,KV,HD,S", SHAPES)
def test_attn_decode_bf16_cache(gpu, NH, KV, HD, S):
    """Per position / row case: the stored row is RNE(bf16) of the row the fp32
    call stores and no other row changes; at position 0 the output is the
    rounded v bit-exactly.  Per shape: the bf16 kernel's error against its own
    float64 reference is within 2 x the fp32-cache kernel's on the same
    inputs (the same fp32 arithmetic in the same order on other operand values)."""
    c = _case(NH, KV, HD)
    gph = NH // KV
    e32 = e16 = 0.0
    for pos in _pos_cases(S):
        rows = len(pos)
        o32, k32, v32, _ = _run(c, S, pos, 0)
        o16, k16, v16, (kb, vb) = _run(c, S, pos, 1)
        assert np.isfinite(o32).all() and np.isfinite(o16).all(), pos
        for r, p in enumerate(pos):
            # the stored row: RNE of what the fp32 cache received, compared as uint16
            np.testing.assert_array_equal(kb[r, p], rne_bf16(k32[r, p]), err_msg=f"K row, pos {pos} row {r}")
            np.testing.assert_array_equal(vb[r, p], rne_bf16(v32[r, p]), err_msg=f"V row, pos {pos} row {r}")
            # (fp32: v is stored as it came)
            np.testing.assert_array_equal(v32[r, p], c.qkv[r, (NH + KV) * HD:])
            # every other row untouched, in both caches and both modes
            keep = np.arange(S) != p
            np.testing.assert_array_equal(kb[r, keep], c.kbits[r, :S][keep])
            np.testing.assert_array_equal(vb[r, keep], c.vbits[r, :S][keep])
            np.testing.assert_array_equal(k32[r, keep], widen(c.kbits[r, :S][keep]))
            np.testing.assert_array_equal(v32[r, keep], widen(c.vbits[r, :S][keep]))
            if p == 0:   # one key: softmax weight exactly 1, the output is the rounded v of the head's kv head
                vr = widen(rne_bf16(c.qkv[r, (NH + KV) * HD:])).reshape(KV, HD)
                for h in range(NH):
                    np.testing.assert_array_equal(o16[r, h * HD:(h + 1) * HD].view(np.uint32),
                                                  vr[h // gph].view(np.uint32), err_msg=f"pos 0, head {h}")
        e32 = max(e32, float(np.abs(o32 - _reference(c, pos, k32, v32)).max()))
        e16 = max(e16, float(np.abs(o16 - _reference(c, pos, k16, v16)).max()))
    _ERRS[(NH, KV, HD, S)] = (e32, e16)
    print(f"attn_decode NH={NH} KV={KV} HD={HD} S={S}: e32 {e32:.3e}  e16 {e16:.3e}  ratio {e16 / e32:.2f}")
    assert e32 > 0 and e16 <= 2 * e32, (e32, e16)


def test_attn_decode_capacity_independent(gpu):
    """position 33 gives the same bits in a 40- and a 320-row cache (another
    split grid, the same live splits), in both modes"""
    c = _case(4, 2, 128)
    for dtype in (0, 1):
        for pos in ([33], [33, 1, 32]):
            a = _run(c, S_SMALL, pos, dtype)[0]
            b = _run(c, S_BIG, pos, dtype)[0]
            np.testing.assert_array_equal(a.view(np.uint32), b.view(np.uint32))


def test_attn_decode_refuses_position_outside_cache(gpu):
    c = _case(4, 2, 32)
    for pos in ([S_SMALL], [-1], [0, S_SMALL, 1]):
        with pytest.raises(RuntimeError):
            _run(c, S_SMALL, pos, 1)


# ------------------------------------------------------------------ model level
def _fresh(preset="tiny", kv=None, **ov):
    m = qtts.QwenTTS(model_dir(preset, **ov))
    if kv is not None:
        m.set_kv_cache(kv)
    return m


@pytest.fixture(scope="module")
def tiny16(gpu):
    m = _fresh("tiny", "bf16")
    yield m
    m.close()


def _capacity(m):
    """rows per slot of the talker cache, probed through get_kv's range check"""
    lo, hi = 1, 1 << 20
    while lo < hi:   # largest S with row S - 1 readable
        mid = (lo + hi + 1) // 2
        try:
            m.get_kv(0, 0, mid - 1, 1)
            lo = mid
        except ValueError:
            hi = mid - 1
    return lo


def _libm_rope(S, HD, theta):
    """the model's RoPE tables, by the runtime's own libm calls (powf, cosf,
    sinf on floats, T.c:97-113), so that they are the same bits"""
    import ctypes as C
    libm = C.CDLL("libm.so.6")
    for f, n in ((libm.powf, 2), (libm.cosf, 1), (libm.sinf, 1)):
        f.restype, f.argtypes = C.c_float, [C.c_float] * n
    half = HD // 2
    cs, sn = np.zeros((S, HD), np.float32), np.zeros((S, HD), np.float32)
    freq = [np.float32(1.0) / np.float32(libm.powf(theta, float(np.float32(2 * i) / np.float32(HD)))) for i in range(half)]
    for p in range(S):
        for i in range(half):
            ang = float(np.float32(p) * freq[i])
            cs[p, i] = cs[p, i + half] = libm.cosf(ang)
            sn[p, i] = sn[p, i + half] = libm.sinf(ang)
    return cs, sn


@pytest.mark.parametrize("preset,nb,frames", [("hd128", 2, 100), ("tiny", 3, 40)])
def test_attn_decode_dtype0_is_the_models_fp32_path(gpu, monkeypatch, preset, nb, frames):
    """kv_dtype 0 through qtts_hip_attn_decode == the model's own fp32 talker
    attention launch, bit for bit: the yardstick e32 above is the model's
    path, wrapper arguments (row strides, split count, scratch, default keys
    per split, own merge) included.  A lock-step batch in fp32 mode (its
    attention merges its own splits, as the entry does); then the last talker
    pass of the last layer is replayed through the entry: the q|k|v rows it
    read (get_attn), the cache rows below its position (get_kv), the layer's
    norm weights and the RoPE tables.  The K / V row it stores and its output
    must equal the model's.  hd128: 32-key splits, position 108 = 4 splits."""
    import torch
    from qtts_io import bf16_to_f32, read_model_tensors
    for k in ("QTTS_HIP_KV", "QTTS_HIP_ATTN_LPK"):
        monkeypatch.delenv(k, raising=False)
    P_LEN = 10   # prompt rows with a speaker and a language (see test_layer0_cache_rows_slot2_of_three)
    md = model_dir(preset)
    m = qtts.QwenTTS(md)
    try:
        ids = [prompt_ids("p128", 1800 + b) for b in range(nb)]
        m.set_params(max_tokens=frames, fixed=frames, seed=4, **DEFAULT)
        rc, _ = m.generate_batch(ids, ["aiden"] * nb, ["english"] * nb)
        assert rc == 0
        cfg = m.cfg
        NH, KV, HD, L = cfg.talker_heads, cfg.talker_kv_heads, cfg.talker_head_dim, cfg.talker_layers
        S = _capacity(m)
        pos = P_LEN + frames - 2   # frame j + 1's talker pass writes row P_LEN + j; the last frame is frames - 1
        qkv, att = m.get_attn(nb)
        rows = [m.get_kv(L - 1, b, 0, pos + 1) for b in range(nb)]
        eps, theta = float(cfg.talker_rms_norm_eps), float(cfg.talker_rope_theta)
    finally:
        m.close()
    kc = np.zeros((nb, S, KV * HD), np.float32)
    vc = np.zeros((nb, S, KV * HD), np.float32)
    for b in range(nb):
        kc[b, :pos], vc[b, :pos] = rows[b][0][:pos], rows[b][1][:pos]   # (row `pos` is the entry's to write)
    tens = read_model_tensors(md)

    def w(name):
        dt, a = tens[f"talker.model.layers.{L - 1}.self_attn.{name}.weight"]
        return np.ascontiguousarray(bf16_to_f32(a) if dt == "BF16" else a, np.float32)
    cs, sn = _libm_rope(S, HD, theta)
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    out = torch.full((nb, NH * HD), float("nan"), dtype=torch.float32, device=dev)
    kcd, vcd = t(kc), t(vc)
    qtts.Kernels.attn_decode(out, t(qkv), kcd, vcd, t(w("q_norm")), t(w("k_norm")), t(cs), t(sn),
                             t(np.full(nb, pos, np.int32)), NH, KV, HD, S, nb, eps, 0)
    torch.cuda.synchronize()
    kg, vg, og = kcd.cpu().numpy(), vcd.cpu().numpy(), out.cpu().numpy()
    assert np.abs(att).max() > 0
    for b in range(nb):
        np.testing.assert_array_equal(kg[b, pos].view(np.uint32), rows[b][0][pos].view(np.uint32), err_msg=f"K row, slot {b}")
        np.testing.assert_array_equal(vg[b, pos].view(np.uint32), rows[b][1][pos].view(np.uint32), err_msg=f"V row, slot {b}")
        np.testing.assert_array_equal(og[b].view(np.uint32), att[b].view(np.uint32), err_msg=f"attention output, slot {b}")
        # (the row is this pass's: v came straight from the q|k|v row)
        np.testing.assert_array_equal(rows[b][1][pos], qkv[b, (NH + KV) * HD:])


@pytest.mark.parametrize("preset,nb", [("tiny", 1), ("tiny", 3), ("hd128", 2)])
def test_state_bytes_drop_by_half_the_cache(gpu, monkeypatch, preset, nb):
    """qtts_dev_bytes(dev, 1) after begin: K and V each save 2 B per element,
    L B S KV HD 4 bytes together.  The allocator counts the bytes asked for,
    one hipMalloc per buffer with no rounding of its own (dalloc in
    qtts_runtime.hip; QTTS_HIP_ARENA, off by default, only carves buffers of
    <= 1 MB out of 32 MB blocks), so the drop is exact."""
    monkeypatch.delenv("QTTS_HIP_ARENA", raising=False)
    monkeypatch.delenv("QTTS_HIP_KV", raising=False)
    m = _fresh(preset)
    try:
        assert m.kv_cache() == qtts.KV_F32
        ids = [prompt_ids("p128", 1500 + b) for b in range(nb)]
        got = {}
        for mode in ("fp32", "bf16"):
            m.set_kv_cache(mode)
            assert m.kv_cache() == (qtts.KV_BF16 if mode == "bf16" else qtts.KV_F32)
            m.set_params(max_tokens=40, fixed=2, seed=1, **GREEDY)
            if nb == 1:
                assert m.generate(ids[0], "aiden", "english") is not None
            else:
                rc, _ = m.generate_batch(ids, ["aiden"] * nb, ["english"] * nb)
                assert rc == 0
            got[mode] = (m.state_bytes(), _capacity(m))
        cfg = m.cfg
        S = got["fp32"][1]
        assert got["bf16"][1] == S and S > 10 + 2, got   # (prompt rows + the fixed frames fit)
        want = cfg.talker_layers * nb * S * cfg.talker_kv_heads * cfg.talker_head_dim * 4
        assert got["fp32"][0] - got["bf16"][0] == want, (got, want)
    finally:
        m.close()


def _stage_run(m, emb, steps):
    m.prefill(emb)
    lg = None
    for e in steps:
        lg, _ = m.step(e)
    k, v = m.get_kv(0, 0, 0, len(emb) + len(steps))
    return k, v, lg


def test_layer0_cache_rows_stage_api(gpu):
    """24-row prefill, then 8 decode steps on fixed embeddings: layer 0's K / V
    depend on the embeddings alone, so its 32 rows in bf16 mode are RNE(bf16)
    of the rows in fp32 mode, bit for bit (the prefill writer, the decode
    writer, and the layer stride: a wrong one lets layer 1 overwrite them).
    The last step's logits differ between the modes by the quantisation, not
    by O(1) (a coarse stride / widening check, not an accuracy bar)."""
    m = _fresh("tiny")
    try:
        rng = np.random.default_rng(77)
        H = m.cfg.talker_hidden
        emb = (rng.standard_normal((24, H)) * 0.5).astype(np.float32)
        steps = (rng.standard_normal((8, H)) * 0.5).astype(np.float32)
        k32, v32, lg32 = _stage_run(m, emb, steps)
        m.set_kv_cache("bf16")
        k16, v16, lg16 = _stage_run(m, emb, steps)
        assert np.abs(k32).max() > 0 and np.abs(v32).max() > 0
        np.testing.assert_array_equal(rne_bf16(k16), rne_bf16(k32))
        np.testing.assert_array_equal(rne_bf16(v16), rne_bf16(v32))
        np.testing.assert_array_equal(k16, widen(rne_bf16(k32)))   # (and get_kv widens exactly)
        np.testing.assert_array_equal(v16, widen(rne_bf16(v32)))
        rel = float(np.linalg.norm(lg16.astype(np.float64) - lg32) / np.linalg.norm(lg32.astype(np.float64)))
        print(f"tiny stage run, last step logits: relative L2 difference bf16 vs fp32 cache {rel:.3e}")
        assert 0 < rel < 0.05, rel
        # back to fp32 on the same context: the fp32 rows again, bit for bit
        m.set_kv_cache("fp32")
        k, v, lg = _stage_run(m, emb, steps)
        np.testing.assert_array_equal(k, k32)
        np.testing.assert_array_equal(v, v32)
        np.testing.assert_array_equal(lg, lg32)
    finally:
        m.close()


def test_layer0_cache_rows_slot2_of_three(gpu):
    """The same as slot 2 of a 3-slot lock-step batch (the slot stride of both
    writers, in the batch kernels).  Rows [0, p_len) come from the prompt
    alone.  Row p_len + j is the talker step on frame j's codes: it is
    compared wherever both modes drew the same frame j (greedy draws; layer
    0's K / V at a position depend on that position's input alone), and frame
    0 at least must be such a frame."""
    P_LEN = 10   # 3 role rows + think, think_bos, language, think_eos, speaker, pad | bos (build_prompt)
    ids = [prompt_ids("p128", 1600 + b) for b in range(3)]
    rows, codes = {}, {}
    m = _fresh("tiny")
    try:
        for mode in ("fp32", "bf16"):
            m.set_kv_cache(mode)
            m.set_params(max_tokens=16, fixed=9, seed=3, **GREEDY)
            rc, _ = m.generate_batch(ids, ["aiden"] * 3, ["english"] * 3)
            assert rc == 0
            codes[mode] = m.last_codes_slot(2, 16)
            rows[mode] = [m.get_kv(0, b, 0, P_LEN + 8) for b in range(3)]
            if mode == "bf16":   # slot 2, every layer
                rows16_all = [m.get_kv(l, 2, 0, P_LEN + 8) for l in range(m.cfg.talker_layers)]
    finally:
        m.close()
    assert codes["fp32"].shape == (9, 16)
    same = [j for j in range(8) if np.array_equal(codes["fp32"][j], codes["bf16"][j])]
    assert 0 in same, (codes["fp32"][0], codes["bf16"][0])
    take = list(range(P_LEN)) + [P_LEN + j for j in same]
    for i in range(2):
        a32, a16 = rows["fp32"][2][i][take], rows["bf16"][2][i][take]
        np.testing.assert_array_equal(a16, widen(rne_bf16(a32)))
    # every row of slot 2 in bf16 mode, decode rows and every layer included,
    # against the same utterance as slot 0 of the same batch in another order
    # (the same batch kernels, so the same arithmetic per row): bit for bit,
    # whatever the fp32 run drew.  Overlapping or misplaced slots differ here.
    # (Against the utterance ALONE this does not hold bit for bit: the batch-1
    # GEMVs sum in another order than the batch ones, and a bf16 rounding tie
    # in a later layer's row can fall the other way -- measured: one V element
    # of layer 1 in 1152, one bf16 ulp.)
    s1 = _fresh("tiny", "bf16")
    try:
        s1.set_params(max_tokens=16, fixed=9, seed=3, **GREEDY)
        rc, _ = s1.generate_batch([ids[2], ids[0], ids[1]], ["aiden"] * 3, ["english"] * 3)
        assert rc == 0
        np.testing.assert_array_equal(s1.last_codes_slot(0, 16), codes["bf16"])
        for l in range(s1.cfg.talker_layers):
            ks, vs = s1.get_kv(l, 0, 0, P_LEN + 8)
            np.testing.assert_array_equal(rows16_all[l][0].view(np.uint32), ks.view(np.uint32), err_msg=f"K, layer {l}")
            np.testing.assert_array_equal(rows16_all[l][1].view(np.uint32), vs.view(np.uint32), err_msg=f"V, layer {l}")
    finally:
        s1.close()
    # the three slots hold three different prompts (a slot stride of 0 would not)
    assert not np.array_equal(rows["bf16"][2][0][:P_LEN], rows["bf16"][1][0][:P_LEN])
    assert not np.array_equal(rows["bf16"][1][0][:P_LEN], rows["bf16"][0][0][:P_LEN])


def test_batch_rows_equal_single_runs_bf16(tiny16):
    """row i of a lock-step batch of 4 == utterance i alone, same seed"""
    m = tiny16
    ids = [prompt_ids("short")] + [prompt_ids("p128", 1700 + b) for b in range(3)]
    m.set_params(max_tokens=64, fixed=24, seed=11, **DEFAULT)
    single = []
    for i in ids:
        assert m.generate(i, "aiden", "english") is not None
        single.append(m.last_codes())
    rc, _ = m.generate_batch(ids, ["aiden"] * 4, ["english"] * 4)
    assert rc == 0 and m.kv_cache() == qtts.KV_BF16
    for b in range(4):
        np.testing.assert_array_equal(m.last_codes_slot(b, 64), single[b], err_msg=f"batch row {b}")


def test_stream_equals_generate_bf16(tiny16):
    m = tiny16
    ids = prompt_ids("p128", 1710)
    m.set_params(max_tokens=64, fixed=24, seed=5, **DEFAULT)
    a = m.generate(ids, "aiden", "english")
    ca = m.last_codes()
    b = m.generate_stream(ids, "aiden", "english", chunk_frames=4)
    np.testing.assert_array_equal(m.last_codes(), ca)
    assert a.shape == b.shape


def test_hd128_300_frames_repeat_and_capacity_bf16(gpu):
    """hd128 (32-key splits), 300 frames in bf16 mode: a second run repeats the
    first; a cache with room for 4096 frames instead of 300 is another split
    grid with the same live splits merged in split order -- the same codes."""
    ids = prompt_ids("p128", 42)
    out = []
    for big in (False, False, True):
        m = _fresh("hd128", "bf16")   # (a fresh context: the capacity never shrinks on a live one)
        try:
            if big:   # the stage API allocates the reference's default capacity (4096 frames); generate keeps it
                m.prefill(np.zeros((2, m.cfg.talker_hidden), np.float32))
            m.set_params(max_tokens=300, fixed=300, seed=42, **DEFAULT)
            assert m.generate(ids, "aiden", "english") is not None
            out.append((m.last_codes(), _capacity(m)))
        finally:
            m.close()
    assert out[0][0].shape == (300, 16)
    assert out[0][1] == out[1][1] < 400 and out[2][1] > 4096, [o[1] for o in out]
    np.testing.assert_array_equal(out[0][0], out[1][0], err_msg="second run")
    np.testing.assert_array_equal(out[0][0], out[2][0], err_msg="capacity 4096 vs 300")


def test_queue_equals_single_runs_bf16(gpu):
    """The tiny EOS model, 6 utterances on 2 slots (refills, tail compaction,
    move_slot, set_rows) in bf16 mode: every utterance equals its own single
    run in the same mode.  A refilled slot runs its last prompt row as a decode
    step (the token's own k / v from LDS) where the single run prefills it
    (read back from the cache): equal only because both see the rounded values."""
    md_args = dict(eos_gain=manifest()["eos_gain"])
    m = _fresh("tiny", "bf16", **md_args)
    try:
        prompts = [prompt_ids("short")] + [prompt_ids("p128", 1310 + i) for i in range(5)]
        m.set_params(max_tokens=32, fixed=0, seed=7, **DEFAULT)
        single = []
        for p in prompts:
            assert m.generate(p, "aiden", "english") is not None
            single.append(m.last_codes())
        rc, audio = m.generate_queue(prompts, ["aiden"] * 6, ["english"] * 6, slots=2)
        assert rc == 0
        st = m.queue_stats()
        assert st["slots"] == 2 and st["refills"] == 4, st
        assert st["rows_launched"] < 2 * st["frames"], st   # the tail ran compacted
        for i in range(6):
            np.testing.assert_array_equal(m.queue_codes(i), single[i], err_msg=f"utterance {i} (slot {st['slot'][i]})")
        assert len({len(s) for s in single}) > 1, "EOS stops of one length only"
    finally:
        m.close()


def test_mode_switch_back_to_fp32_reproduces_fresh_context(gpu):
    """bf16 -> fp32 on one context, then generating again: the codes of a fresh
    fp32 context (the state is reallocated and the frame graphs recaptured)."""
    ids = prompt_ids("p128", 1720)
    par = dict(max_tokens=64, fixed=24, seed=9, **DEFAULT)
    f = _fresh("tiny")
    try:
        f.set_params(**par)
        f.generate(ids, "aiden", "english")
        want = f.last_codes()
    finally:
        f.close()
    m = _fresh("tiny", "bf16")
    try:
        m.set_params(**par)
        m.generate(ids, "aiden", "english")
        c16 = m.last_codes()
        m.set_kv_cache("fp32")
        m.generate(ids, "aiden", "english")
        np.testing.assert_array_equal(m.last_codes(), want)
        m.set_kv_cache("bf16")
        m.generate(ids, "aiden", "english")
        np.testing.assert_array_equal(m.last_codes(), c16)
    finally:
        m.close()


def test_env_default_selects_bf16(gpu, monkeypatch):
    """QTTS_HIP_KV=bf16 at load == set_kv_cache("bf16")"""
    ids = prompt_ids("p128", 1730)
    par = dict(max_tokens=32, fixed=12, seed=2, **DEFAULT)
    monkeypatch.setenv("QTTS_HIP_KV", "bf16")
    e = _fresh("tiny")
    monkeypatch.delenv("QTTS_HIP_KV")
    m = _fresh("tiny", "bf16")
    try:
        assert e.kv_cache() == qtts.KV_BF16
        for x in (e, m):
            x.set_params(**par)
            x.generate(ids, "aiden", "english")
        np.testing.assert_array_equal(e.last_codes(), m.last_codes())
        assert e.state_bytes() == m.state_bytes()
    finally:
        e.close()
        m.close()
