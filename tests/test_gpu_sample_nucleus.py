"""The nucleus short list (k_sample_n.hip; qtts_sample_dev.h sample_nucleus):
top_p < 1 with top_k <= 64 or top-k off draws from at most 64 ids and one
sequential sum over the vocabulary, and falls back to the full path inside the
launch when the short list cannot decide.

The truth is the CPU oracle's orc_sample (K.c:407-558 restated); ids and RNG
states are bit-equal everywhere.  `path` says which path a row ran (1 fast
top-k, 2 nucleus short list, 3 full), so that a kernel that always falls back
cannot pass:

1. rows the short list must take (path 2): random rows a float64 check finds
   decidable, and the shapes that go wrong first (ties at the threshold, 1 ulp
   apart, the suppression block, -FLT_MAX, +-0, no cut);
2. rows that must fall back (path 3) and still be bit-equal;
3. the two RNG edges, r = 0 and r = 1;
4. the fixed-mode EOS redraw;
5. plain entry == rows entry, QTTS_HIP_SAMPLE_NUCLEUS=0, mixed launches;
6. the tiny model: ctx-wide nucleus, one armed nucleus row in a batch, a fed
   stream.
"""
import ctypes as C

import numpy as np
import pytest

from conftest import model_dir
from oracle_py import DEFAULT, Oracle, fptr
from qtts_io import lookup_ids
from synth_model import prompt_ids

import qtts

pytestmark = pytest.mark.gpu

FMAX = float(np.finfo(np.float32).max)
VS = (64, 100, 1500, 2048, 3072, 4096)
PS = (1e-6, 0.5, 0.8, 0.9, 0.99)


def T(a, dev, dtype=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.view(dtype)
    return t.to(dev)


def bits(st):
    """RNG states as uint32 bit patterns (a float32 array is reinterpreted)"""
    a = np.asarray(st)
    return a.view(np.uint32) if a.dtype == np.float32 else a.astype(np.uint32)


def run_rows(dev, lg, rows, st0, eos=-1, redraw=False):
    """the rows entry: (ids, RNG state bits, path) per row"""
    import torch
    B, V = lg.shape
    out = torch.full((B,), -7, dtype=torch.int32, device=dev)
    path = torch.full((B,), -7, dtype=torch.int32, device=dev)
    rs = T(bits(st0).view(np.int32), dev)
    qtts.Kernels.sample_nucleus_rows(out, path, T(lg, dev), V, [r[0] for r in rows], [r[1] for r in rows],
                                     [r[2] for r in rows], rs, B, eos=eos, redraw=redraw)
    torch.cuda.synchronize()
    return out.cpu().numpy(), rs.cpu().numpy().view(np.uint32), path.cpu().numpy()


def orc(oracle, lg_row, row, st_bits):
    """orc_sample on one row: (id, RNG state bits after)"""
    s = np.array([st_bits], np.uint32).view(np.float32)
    e = oracle.lib.orc_sample(fptr(np.ascontiguousarray(lg_row, np.float32).copy()), len(lg_row), int(row[0]),
                              float(row[1]), float(row[2]), fptr(s))
    return e, int(s.view(np.uint32)[0])


def check(oracle, lg, rows, st0, got, want_path, what):
    r, st, path = got
    sb = bits(st0)
    for b, row in enumerate(rows):
        e, s = orc(oracle, lg[b], row, sb[b])
        assert r[b] == e, (what, b, row, int(r[b]), e)
        assert st[b] == s, (what, b, row)
        if want_path is not None:
            assert path[b] == want_path, (what, b, row, int(path[b]))


def decidable(lg_row, row, margin=1e-5):
    """float64: the short list can decide this row.  top-k on (0 < k < V, k <=
    64): the k-th scaled logit lies within 80 of the maximum, at most 64
    probabilities reach the k-th and the next one below is more than `margin`
    (relative) smaller; top-k off: the 64 largest hold more than top_p of the
    mass, with 1e-3 to spare."""
    k, tp, temp = row
    V = len(lg_row)
    v = lg_row.astype(np.float64) / max(float(np.float32(temp)), 1e-5)
    if not np.isfinite(v.max()):
        return False
    p = np.exp(v - v.max())
    p /= p.sum()
    srt = np.sort(p)[::-1]
    if 0 < k < V:
        if k > 64 or not (v.max() - np.sort(v)[::-1][k - 1] < 80.0):
            return False
        ns = int((p >= srt[k - 1]).sum())
        return ns <= 64 and (ns == V or srt[ns] < srt[k - 1] * (1.0 - margin))
    return srt[:64].sum() > tp + 1e-3


# ---------------------------------------------------------------- 1. must be nucleus-short
def random_launches():
    """launches of 1, 3 and 8 rows with mixed parameters, every row decidable"""
    rng = np.random.default_rng(20251)
    out = []
    for V in VS:
        ks = [1, 2, 50, 63, 64, 0, V]
        for B in (1, 3, 8):
            for it in range(4):
                lg = np.zeros((B, V), np.float32)
                rows = []
                for b in range(B):
                    for attempt in range(200):
                        row = (int(ks[int(rng.integers(0, len(ks)))]), float(PS[int(rng.integers(0, len(PS)))]),
                               float(rng.uniform(0.4, 1.7)))
                        # top-k off needs a peaked row for 64 ids to hold top_p of the mass
                        lo = 3.0 if not 0 < row[0] < V else 0.5
                        x = (rng.standard_normal(V) * rng.uniform(lo, 8.0)).astype(np.float32)
                        if decidable(x, row):
                            break
                    else:
                        raise AssertionError(("no decidable row", V, B, it, b))
                    lg[b] = x
                    rows.append(row)
                out.append((lg, rows, rng.integers(1, 10**6, B).astype(np.float32)))
    return out


def test_random_rows_take_the_short_list(gpu, oracle):
    launches = random_launches()
    n = sum(len(rows) for _, rows, _ in launches)
    assert n >= 200, n
    seen = {(0 < r[0] < lg.shape[1], r[1]) for lg, rows, _ in launches for r in rows}
    assert len(seen) == 2 * len(PS), seen   # top-k on and off at every top_p
    for i, (lg, rows, st0) in enumerate(launches):
        check(oracle, lg, rows, st0, run_rows(gpu, lg, rows, st0), 2, ("random", i, lg.shape))


def _special_rows():
    """(name, logits row, (k, top_p, T)) -- each decidable with <= 64 survivors"""
    rng = np.random.default_rng(77)
    out = []
    for c in (3, 4, 6):   # c extra exact copies of the k-th logit: survivors k + c
        for V, k in ((2048, 50), (3072, 50), (100, 2)):
            x = (rng.standard_normal(V) * 3.0).astype(np.float32)
            order = np.argsort(-x, kind="stable")
            x[order[k:k + c]] = x[order[k - 1]]
            out.append((f"{c} copies of the k-th logit, V {V}", x, (k, 0.9, 0.8)))
    for V, k, tp in ((2048, 50, 0.99), (1500, 63, 0.8), (4096, 2, 0.99)):   # 1 ulp apart at the threshold
        x = (rng.standard_normal(V) * 2.0).astype(np.float32)
        order = np.argsort(-x, kind="stable")
        x[order[k]] = np.nextafter(x[order[k - 1]], np.float32(-np.inf))
        out.append((f"1 ulp below the k-th logit, V {V}", x, (k, tp, 1.1)))
    for tp, temp in ((0.8, 0.9), (0.5, 1.3)):   # the talker's suppression: the last 1024 ids at -1e9 except one
        x = (rng.standard_normal(3072) * 3.0).astype(np.float32)
        keep = x[2150]
        x[2048:] = -1e9
        x[2150] = keep + 4.0
        out.append(("suppressed block", x, (50, tp, temp)))
        out.append(("suppressed block, top-k off", x * 2.0, (0, tp, temp)))
    for temp in (0.5, 1.5):   # -FLT_MAX entries (-inf after the division below T = 1)
        x = (rng.standard_normal(2048) * 8.0).astype(np.float32)
        x[rng.integers(0, 2048, 700)] = -FMAX
        out.append(("-FLT_MAX entries", x, (64, 0.9, temp)))
        out.append(("-FLT_MAX entries, top-k off", x, (2048, 0.9, temp)))
    for V in (100, 1500):   # +0 / -0 mixed under a few distinct positive logits
        x = np.where(rng.integers(0, 2, V) == 1, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
        top = rng.choice(V, 40, replace=False)
        x[top] = (np.arange(40) * 0.37 + 9.0 + rng.uniform(0, 0.1, 40)).astype(np.float32)
        out.append((f"+-0 mixture, V {V}", x, (30, 0.9, 1.0)))
        out.append((f"+-0 mixture, top-k off, V {V}", x, (0, 0.9, 1.0)))
    for V, k in ((3072, 50), (2048, 64)):   # the top-k mass stays below top_p: nothing is cut
        x = (rng.standard_normal(V) * 0.3).astype(np.float32)
        out.append((f"no cut, V {V}", x, (k, 0.9, 1.0)))
    return out


def test_special_rows_take_the_short_list(gpu, oracle):
    cases = _special_rows()
    for name, x, row in cases:
        assert decidable(x, row, margin=0.0 if "ulp" in name else 1e-5), name
        if "no cut" in name:   # the precondition the name states, in float64
            v = x.astype(np.float64) / row[2]
            p = np.exp(v - v.max())
            assert np.sort(p)[::-1][:row[0]].sum() / p.sum() < row[1] - 0.1, name
    rng = np.random.default_rng(3)
    for name, x, row in cases:
        lg = x[None, :].copy()
        st0 = rng.integers(1, 10**6, 1).astype(np.float32)
        check(oracle, lg, [row], st0, run_rows(gpu, lg, [row], st0), 2, name)


# ---------------------------------------------------------------- 2. must fall back
def test_rows_that_fall_back(gpu, oracle):
    rng = np.random.default_rng(11)
    cases = []
    x = (rng.standard_normal(2048) * 3.0).astype(np.float32)
    order = np.argsort(-x, kind="stable")
    x[order[50:130]] = x[order[49]]
    cases.append(("80 copies of the k-th logit", x, (50, 0.9, 0.9)))
    cases.append(("every logit equal", np.full(1500, 1.25, np.float32), (50, 0.8, 1.0)))
    cases.append(("every logit equal, top-k off", np.full(1500, 1.25, np.float32), (0, 0.8, 1.0)))
    y = (rng.standard_normal(3072) * 3.0).astype(np.float32)
    cases.append(("T = 1e-5: the k-th p underflows", y, (50, 0.9, 1e-5)))
    cases.append(("T = 0", y, (50, 0.9, 0.0)))
    z = rng.standard_normal(3072).astype(np.float32)
    cases.append(("top-k off at T = 50: the cut lies past 64", z, (0, 0.9, 50.0)))
    cases.append(("k = 65", y, (65, 0.9, 0.9)))
    cases.append(("k = 300", y, (300, 0.8, 0.9)))
    for name, x, row in cases:
        for seed in (5.0, 123456.0):
            lg = x[None, :].copy()
            st0 = np.array([seed], np.float32)
            check(oracle, lg, [row], st0, run_rows(gpu, lg, [row], st0), 3, name)


# ---------------------------------------------------------------- 3. the RNG edges
def _xs(s):
    s ^= (s << 13) & 0xFFFFFFFF
    s ^= s >> 17
    s ^= (s << 5) & 0xFFFFFFFF
    return s


def _xs_inv(s):
    """the state whose xorshift32 successor is s: the three shifts undone in reverse"""
    def unl(x, a):
        y, t = x, (x << a) & 0xFFFFFFFF
        while t:
            y ^= t
            t = (t << a) & 0xFFFFFFFF
        return y

    def unr(x, a):
        y, t = x, x >> a
        while t:
            y ^= t
            t >>= a
        return y
    return unl(unr(unl(s, 5), 17), 13)


def test_rng_edges(gpu, oracle):
    """r = 0 (the successor's low 31 bits are 0) returns id 0 whether or not id
    0 is kept; r = 1.0 against a sum rounded below 1 returns 0 as well"""
    edges = []
    for succ, r in ((0x80000000, 0.0), (0x7FFFFFFF, 1.0), (0xFFFFFFFF, 1.0)):
        s0 = _xs_inv(succ)
        assert _xs(s0) == succ and s0 != 0
        assert np.float32(succ & 0x7FFFFFFF) / np.float32(0x7FFFFFFF) == np.float32(r)
        edges.append((s0, r))
    rng = np.random.default_rng(8)
    for V, row in ((2048, (50, 0.8, 0.9)), (3072, (0, 0.9, 0.7)), (100, (2, 0.5, 1.0)), (1500, (64, 0.99, 1.2))):
        for zero_kept in (True, False):
            x = (rng.standard_normal(V) * 4.0).astype(np.float32)
            x[0] = x.max() + 1.0 if zero_kept else -40.0
            assert decidable(x, row)
            for s0, r in edges:
                lg = x[None, :].copy()
                st0 = np.array([s0], np.uint32)
                got = run_rows(gpu, lg, [row], st0)
                check(oracle, lg, [row], st0, got, 2, (V, row, zero_kept, r))
                if r == 0.0:
                    assert got[0][0] == 0


# ---------------------------------------------------------------- 4. the redraw
def test_eos_redraw(gpu, oracle):
    """talker mode before the fixed length: a row whose nucleus draw is the EOS
    id draws again with that logit at -1e9 and the state carried over; the
    other rows are what they were"""
    rng = np.random.default_rng(21)
    B, V, eos = 8, 2048, 1999
    rows = [((50, 0.8, 0.9), (0, 0.9, 0.6), (64, 0.5, 1.2), (2, 0.99, 1.0))[b % 4] for b in range(B)]
    base = (rng.standard_normal((B, V)) * 4.0).astype(np.float32)
    st0 = rng.integers(1, 10**6, B).astype(np.float32)
    for bump in np.arange(-1.0, 6.0, 0.25):   # raise the EOS logit until about half the rows draw it
        lg = base.copy()
        lg[:, eos] = base.max(axis=1) + np.float32(bump)
        first = [orc(oracle, lg[b], rows[b], bits(st0)[b]) for b in range(B)]
        hit = [e == eos for e, _ in first]
        if 3 <= sum(hit) <= 5:
            break
    assert 3 <= sum(hit) <= 5, hit
    want = []
    for b in range(B):
        e, s = first[b]
        if hit[b]:
            x = lg[b].copy()
            x[eos] = -1e9
            assert decidable(x, rows[b])
            e, s = orc(oracle, x, rows[b], s)
        assert decidable(lg[b], rows[b])
        want.append((e, s))
    r, st, path = run_rows(gpu, lg, rows, st0, eos=eos, redraw=True)
    for b in range(B):
        assert (int(r[b]), int(st[b])) == want[b], (b, hit[b], rows[b], int(r[b]), want[b][0])
        assert path[b] == 2, (b, int(path[b]))
    # without the redraw the EOS rows keep their EOS
    r, st, path = run_rows(gpu, lg, rows, st0)
    for b in range(B):
        assert (int(r[b]), int(st[b])) == first[b], b


# ---------------------------------------------------------------- 5. equivalences
def _run_plain(dev, lg, row, st0):
    import torch
    B, V = lg.shape
    out = torch.full((B,), -7, dtype=torch.int32, device=dev)
    path = torch.full((B,), -7, dtype=torch.int32, device=dev)
    rs = T(bits(st0).view(np.int32), dev)
    qtts.Kernels.sample_nucleus(out, T(lg, dev), V, row[0], row[1], row[2], rs, B, path_i32=path)
    torch.cuda.synchronize()
    return out.cpu().numpy(), rs.cpu().numpy().view(np.uint32), path.cpu().numpy()


def _decidable_batch(rng, B, V, row, scale):
    lg = np.zeros((B, V), np.float32)
    for b in range(B):
        for attempt in range(200):
            lg[b] = (rng.standard_normal(V) * scale).astype(np.float32)
            if decidable(lg[b], row):
                break
        else:
            raise AssertionError(("no decidable row", V, row))
    return lg


@pytest.mark.parametrize("V", [2048, 3072])
def test_plain_entry_equals_rows_entry_and_the_switch(gpu, oracle, monkeypatch, V):
    rng = np.random.default_rng(V)
    B = 8
    for row in ((50, 0.8, 0.9), (0, 0.7, 0.8), (64, 0.99, 1.4)):
        lg = _decidable_batch(rng, B, V, row, 4.0)
        st0 = rng.integers(1, 10**6, B).astype(np.float32)
        a = _run_plain(gpu, lg, row, st0)
        b = run_rows(gpu, lg, [row] * B, st0)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes(), row
        check(oracle, lg, [row] * B, st0, a, 2, ("plain", row))
        # the plain sampler entry routes such parameters to the same kernel
        import torch
        out = torch.zeros(B, dtype=torch.int32, device=gpu)
        rs = T(bits(st0).view(np.int32), gpu)
        qtts.Kernels.sample_top_k(out, T(lg, gpu), V, row[0], row[1], row[2], rs, B)
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == a[0].tobytes() and rs.cpu().numpy().tobytes() == a[1].tobytes()
        monkeypatch.setenv("QTTS_HIP_SAMPLE_NUCLEUS", "0")
        try:
            a0 = _run_plain(gpu, lg, row, st0)
            b0 = run_rows(gpu, lg, [row] * B, st0)
        finally:
            monkeypatch.delenv("QTTS_HIP_SAMPLE_NUCLEUS")
        for got in (a0, b0):
            assert got[0].tobytes() == a[0].tobytes() and got[1].tobytes() == a[1].tobytes(), row
            assert (got[2] == 3).all(), got[2]


def test_mixed_launch_rows_equal_their_single_launches(gpu, oracle):
    """fast, nucleus-short and full rows in one launch: each row's id, state
    and path are those of its own one-row launch"""
    rng = np.random.default_rng(4)
    for V in (1500, 3072):
        kinds = [((50, 1.0, 0.9), 1), ((50, 0.8, 0.9), 2), ((300, 0.9, 0.7), 3), ((0, 0.9, 0.6), 2),
                 ((7, 1.0, 1.3), 1), ((65, 0.5, 1.0), 3), ((0, 1.0, 1.1), 3), ((1, 0.5, 1.0), 2)]
        rows = [k for k, _ in kinds]
        lg = np.concatenate([_decidable_batch(rng, 1, V, row, 4.0) if p == 2 else
                             (rng.standard_normal((1, V)) * 4.0).astype(np.float32) for row, p in kinds])
        st0 = rng.integers(1, 10**6, len(rows)).astype(np.float32)
        got = run_rows(gpu, lg, rows, st0)
        check(oracle, lg, rows, st0, got, None, ("mixed", V))
        assert got[2].tolist() == [p for _, p in kinds], got[2]
        for b, row in enumerate(rows):
            one = run_rows(gpu, lg[b:b + 1], [row], st0[b:b + 1])
            assert (one[0][0], one[1][0], one[2][0]) == (got[0][b], got[1][b], got[2][b]), (V, b, row)


# ---------------------------------------------------------------- 6. the tiny model
NUCLEUS = dict(top_p=0.8, st_top_p=0.7)
FRAMES = 6


def _sampler_names(m, step):
    L = qtts.lib()
    L.qtts_dev_profile_frame.restype = C.c_int
    L.qtts_dev_profile_frame.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    n_max = 4096
    kind, byt, ms = (C.c_int * n_max)(), (C.c_double * n_max)(), (C.c_float * n_max)()
    names = C.create_string_buffer(n_max * 64)
    n = L.qtts_dev_profile_frame(m.c.hip, step, n_max, kind, byt, ms, names)
    assert 0 < n <= n_max, n
    return [names.raw[i * 64:(i + 1) * 64].split(b"\0", 1)[0].decode() for i in range(n) if kind[i] == 3]


def test_model_ctx_wide_nucleus(tts_tiny, oracle):
    """top_p 0.8 / 0.7 for the whole context: the oracle's codes, every sampler
    launch of a frame is the short-list kernel, and none counts as per-slot"""
    m, o = tts_tiny, oracle
    ids = prompt_ids("short")
    pp = dict(DEFAULT, **NUCLEUS)
    n0 = qtts.Kernels.sample_slot_launches()
    m.set_params(max_tokens=4096, fixed=FRAMES, seed=5, **pp)
    assert m.generate(ids, "aiden", "english") is not None
    got = m.last_codes()
    s, l = lookup_ids(o.cfg, "aiden", "english")
    want, _ = o.generate_codes(ids, s, l, max_tokens=4096, fixed=FRAMES, seed=5, **pp)
    np.testing.assert_array_equal(got, want)
    for step in (0, 1):
        names = _sampler_names(m, step)
        assert len(names) == m.cfg.num_code_groups, names   # the talker's draw and the sub-talker's 15
        assert all(nm.startswith("k_sample_n<false") for nm in names), names
    assert qtts.Kernels.sample_slot_launches() == n0
    m.set_params(max_tokens=4096, fixed=FRAMES, seed=5, **DEFAULT)


def test_model_batch_with_one_nucleus_row(tts_tiny, oracle):
    m, o = tts_tiny, oracle
    prompts = [prompt_ids("short"), prompt_ids("p128", 1300), prompt_ids("p128", 1301)]
    per = [dict(seed=7), dict(NUCLEUS, seed=8), dict(seed=9)]
    m.set_params(max_tokens=4096, fixed=FRAMES, seed=42, **DEFAULT)
    n0 = qtts.Kernels.sample_slot_launches()
    m.set_utterance_sampling(per)
    rc, _ = m.generate_batch(prompts, ["aiden"] * 3, ["english"] * 3)
    assert rc == 0 and qtts.Kernels.sample_slot_launches() > n0
    got = m.last_codes_batch(3, FRAMES)
    s, l = lookup_ids(o.cfg, "aiden", "english")
    for b in range(3):
        pp = dict(DEFAULT)
        pp.update({k: v for k, v in per[b].items() if k != "seed"})
        want, _ = o.generate_codes(prompts[b], s, l, max_tokens=4096, fixed=FRAMES, seed=per[b]["seed"], **pp)
        np.testing.assert_array_equal(got[b], want, err_msg=f"slot {b}")


def _fed_codes(m, ids, sampling):
    sent = []

    def feed(h, wait):
        if not sent:
            assert h.push(0, ids) == 0 and h.close(0) == 0
            sent.append(1)
    m.set_params(max_tokens=4096, fixed=FRAMES, seed=42, **DEFAULT)
    m.set_utterance_sampling([sampling])
    assert m.generate_fed_stream(feed, "aiden", "english", chunk_frames=2) is not None
    return m.last_codes_slot(0, FRAMES)


def test_model_fed_stream_nucleus_row(tts_tiny, tiny_dir, monkeypatch):
    """the gated form: a fed stream armed with a nucleus row draws what the
    full-path kernels draw from the same logits (QTTS_HIP_SAMPLE_NUCLEUS=0 on a
    context of its own, so that no captured frame is shared), and differs from
    the default row's run"""
    ids = list(prompt_ids("p128", 1300)[3:-5])
    row = dict(NUCLEUS, seed=8)
    got = _fed_codes(tts_tiny, ids, row)
    other = _fed_codes(tts_tiny, ids, dict(seed=8))
    assert got.shape == (FRAMES, tts_tiny.cfg.num_code_groups) and not np.array_equal(got, other)
    monkeypatch.setenv("QTTS_HIP_SAMPLE_NUCLEUS", "0")
    m0 = qtts.QwenTTS(tiny_dir)
    try:
        want = _fed_codes(m0, ids, row)
    finally:
        m0.close()
        monkeypatch.delenv("QTTS_HIP_SAMPLE_NUCLEUS")
    np.testing.assert_array_equal(got, want)
