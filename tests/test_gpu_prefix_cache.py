"""The instruct prefix cache of the device layer (include/qtts_hip.h): the K / V
rows of a prompt's instruct prefix are computed once per distinct prefix, saved,
and copied back on every later admission.

What must hold, and why it can:
 - a slot with a prefix always takes two passes -- the prefix rows alone, then
   the remaining rows -- whether the prefix was computed or restored, and save /
   restore are plain copies: a hit, a miss and a miss after an eviction leave
   bit-identical KV rows, codes and audio;
 - the prefix pass is over that prefix alone, so its rows do not depend on the
   slot, on the neighbours or on the rest of the prompt: bit-equal across slots
   and against the single run.  The REMAINING rows share one pass with the
   other slots' rows, and the projection kernel follows that pass's row count
   (<= 16 rows or more), so for them the bar across batch shapes is the codes;
 - against the one-pass baseline (cache off) the arithmetic differs only in
   which kernel serves which row count: the stage bar allclose(1e-4, 1e-4) on
   the hidden state after prefill and frame 0's logits, and the baseline's codes
   equal the oracle's.
Both KV element types; `tiny` (KV rows of 64 elements) and `hd128` (1024).
"""
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import manifest, model_dir
from instruct_layout import layout
from oracle_py import DEFAULT, Oracle
from parity import codes_equal
from qtts_io import lookup_ids
from synth_model import prompt_ids

import qtts

pytestmark = pytest.mark.gpu

POOL = np.random.Generator(np.random.PCG64(77)).integers(1000, 100000, size=128).tolist()
IDS = prompt_ids("short")
P_LEN = 10   # aiden / english (checked in _models)


def ins(n, off=0):
    return POOL[off:off + n]


class GenParams(C.Structure):   # qtts_gen_params_t
    _fields_ = [("temperature", C.c_float), ("top_p", C.c_float), ("repetition_penalty", C.c_float),
                ("top_k", C.c_int), ("st_temperature", C.c_float), ("st_top_p", C.c_float), ("st_top_k", C.c_int),
                ("fixed_codec_tokens", C.c_int), ("seed", C.c_int)]


_MODELS = {}


@pytest.fixture(scope="module")
def models(gpu):
    yield _MODELS
    for m, o, _ in _MODELS.values():
        m.close()
        o.close()
    _MODELS.clear()


def _model(models, preset):
    if preset not in models:
        md = model_dir(preset)
        with open(os.path.join(md, "config.json")) as f:
            cfg = json.load(f)
        models[preset] = (qtts.QwenTTS(md), Oracle(md), cfg)
        o = models[preset][1]
        s, l = lookup_ids(o.cfg, "aiden", "english")
        assert o.build_prompt(IDS, s, l)[0].shape[0] == P_LEN
    return models[preset]


def _entry_bytes(m, n, dtype):
    c = m.cfg
    return 2 * c.talker_layers * n * c.talker_kv_heads * c.talker_head_dim * (2 if dtype == "bf16" else 4)


def _kv(m, p_len, b=0, pos0=0):
    return [m.get_kv(l, b, pos0, p_len - pos0) for l in range(m.cfg.talker_layers)]


def _same_kv(a, b, what):
    for l, ((ka, va), (kb, vb)) in enumerate(zip(a, b)):
        np.testing.assert_array_equal(ka, kb, err_msg=f"{what}: K of layer {l}")
        np.testing.assert_array_equal(va, vb, err_msg=f"{what}: V of layer {l}")


def _run(m, instruct, frames=4, seed=9):
    """one armed generate: (codes, audio, KV rows [0, p_len) of every layer, counter deltas)"""
    m.set_params(max_tokens=4096, fixed=frames, seed=seed, **DEFAULT)
    c0 = m.prefix_counters()
    m.set_utterance_instruct([instruct])
    audio = m.generate(IDS, "aiden", "english")
    assert audio is not None
    c1 = m.prefix_counters()
    return m.last_codes(), audio, _kv(m, P_LEN + len(instruct)), tuple(b - a for a, b in zip(c0, c1))


def _want(o, instruct, frames, seed):
    s, l = lookup_ids(o.cfg, "aiden", "english")
    pre, tr = o.build_prompt(IDS, s, l)
    pre = np.concatenate([np.stack([o.embed_text(i) for i in instruct]), pre])
    return o.generate_from_prompt(pre, tr, max_tokens=4096, fixed=frames, seed=seed, **DEFAULT)[0]


# ---------------------------------------------------------------- 1. hit equals miss, bitwise
@pytest.mark.parametrize("n", [1, 7, 40])   # 1 row; <= 16 rows; > 16 rows with a remainder of 10
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
@pytest.mark.parametrize("preset", ["tiny", "hd128"])
def test_hit_equals_miss_bitwise(models, preset, dtype, n):
    m, o, _ = _model(models, preset)
    m.set_kv_cache(dtype)
    m.prefix_cache(0)
    assert m.prefix_cache_bytes() == 0
    m.prefix_cache(16)
    try:
        p = P_LEN + n
        miss = _run(m, ins(n))
        assert miss[3] == (0, 1, p), miss[3]                   # the prefix pass (n rows) + the rest
        assert m.prefix_cache_bytes() == _entry_bytes(m, n, dtype)
        hit = _run(m, ins(n))
        assert hit[3] == (1, 0, p - n), hit[3]                 # a hit sends n fewer rows
        m.prefix_cache(1)                                      # (the one entry stays)
        other = _run(m, ins(n + 2, 50))                        # another prefix evicts it
        assert other[3] == (0, 1, P_LEN + n + 2) and m.prefix_cache_bytes() == _entry_bytes(m, n + 2, dtype)
        again = _run(m, ins(n))
        assert again[3] == (0, 1, p), again[3]
        for name, r in (("hit", hit), ("after eviction", again)):
            np.testing.assert_array_equal(r[0], miss[0], err_msg=name)
            np.testing.assert_array_equal(r[1], miss[1], err_msg=name)
            _same_kv(r[2], miss[2], name)
        if dtype == "fp32":
            codes_equal(miss[0], _want(o, ins(n), 4, 9), f"{preset} prefix of {n}")
        m.prefix_cache(16)
        two = _entry_bytes(m, n, dtype)
        assert m.prefix_cache_bytes() == two                   # (raising the capacity drops nothing)
        _run(m, ins(n + 2, 50))
        assert m.prefix_cache_bytes() == two + _entry_bytes(m, n + 2, dtype)   # the sum over the entries
        m.prefix_cache(0)
        assert m.prefix_cache_bytes() == 0
        off = _run(m, ins(n))
        assert off[3] == (0, 0, p)                             # cache off: ordinary rows of the one pass
    finally:
        m.prefix_cache(16)
        m.set_kv_cache("fp32")


# ---------------------------------------------------------------- 2. restored rows are exact
@pytest.mark.parametrize("dtype", ["fp32", "bf16"])
def test_two_slots_share_a_prefix_and_a_third_is_untouched(models, dtype):
    """slots 0 and 1: the same 7-row prefix under different texts, one computed,
    one restored in the same prefill; slot 2: a 40-row prefix of its own.  The
    one pass over the remaining rows has 30 rows (the > 16-row kernel behind a
    <= 16-row prefix)."""
    m, o, _ = _model(models, "tiny")
    m.set_kv_cache(dtype)
    m.prefix_cache(0)
    m.prefix_cache(16)
    try:
        prompts = [IDS, prompt_ids("p128", 1300), IDS]
        per = [ins(7), ins(7), ins(40, 60)]
        single = _run(m, per[2], frames=4, seed=9)
        m.prefix_cache(0)
        m.prefix_cache(16)
        m.set_params(max_tokens=4096, fixed=4, seed=9, **DEFAULT)
        c0 = m.prefix_counters()
        m.set_utterance_instruct(per)
        rc, _ = m.generate_batch(prompts, ["aiden"] * 3, ["english"] * 3)
        assert rc == 0
        d = tuple(b - a for a, b in zip(c0, m.prefix_counters()))
        assert d == (1, 2, 7 + 40 + 3 * P_LEN), d              # two distinct prefixes computed, one restore
        _same_kv(_kv(m, 7, b=0), _kv(m, 7, b=1), "the shared prefix")
        _same_kv(_kv(m, 40, b=2), [(k[:40], v[:40]) for k, v in single[2]], "the third slot's prefix")
        codes = m.last_codes_batch(3)
        np.testing.assert_array_equal(codes[2][:4], single[0])
        if dtype == "fp32":
            for b in range(3):
                s, l = lookup_ids(o.cfg, "aiden", "english")
                pre, tr = o.build_prompt(prompts[b], s, l)
                pre = np.concatenate([np.stack([o.embed_text(i) for i in per[b]]), pre])
                want = o.generate_from_prompt(pre, tr, max_tokens=4096, fixed=4, seed=9, **DEFAULT)[0]
                codes_equal(codes[b][:4], want, f"slot {b}")
    finally:
        m.set_kv_cache("fp32")


# ---------------------------------------------------------------- 3. against the one-pass baseline
def _device_prefill(m, cfg, instruct, malformed=None):
    """begin / prompt / prefill / frame 0 on the ctx's device model, driven directly:
    (hidden after prefill, frame 0's logits as its code-0 draw saw them)"""
    lib, dev = qtts.lib(), C.c_void_p(m.c.hip)
    text, plan, p_len, ntr = layout(cfg, IDS, "aiden", "english", instruct, 0)
    if malformed:
        malformed(plan)
    gp = GenParams(0.9, 1.0, 1.05, 50, 0.9, 1.0, 50, 2, 9)
    assert lib.qtts_dev_begin(dev, 1, 2, 64, C.byref(gp)) == 0
    flat = [v for row in plan for v in row]
    rc = lib.qtts_dev_prompt(dev, 0, (C.c_int * len(text))(*text), len(text), (C.c_int * len(flat))(*flat), len(plan),
                             p_len, ntr, 3)
    if rc != 0:
        return rc
    assert lib.qtts_dev_tap(dev, 0, 0, 0) == 0
    assert lib.qtts_dev_prefill(dev) == 0
    hid = np.zeros(m.cfg.talker_hidden, np.float32)
    assert lib.qtts_dev_get_hidden(dev, 0, hid.ctypes.data_as(C.POINTER(C.c_float))) == 0
    assert lib.qtts_dev_frame(dev, 0) == 0 and lib.qtts_dev_poll(dev, None, None, None) == 0
    V = m.cfg.talker_vocab_size
    lg = np.zeros(V, np.float32)
    assert lib.qtts_dev_get_tap(dev, 0, lg.ctypes.data_as(C.POINTER(C.c_float)), V, None, None) > 0
    return hid, lg


@pytest.mark.parametrize("n", [1, 7, 40])
@pytest.mark.parametrize("preset", ["tiny", "hd128"])
def test_two_passes_against_one_pass(models, preset, n):
    m, o, cfg = _model(models, preset)
    m.set_kv_cache("fp32")
    try:
        m.prefix_cache(0)
        base = _device_prefill(m, cfg, ins(n))                 # the one-pass baseline
        off = _run(m, ins(n))
        codes_equal(off[0], _want(o, ins(n), 4, 9), f"{preset} one pass, prefix of {n}")
        m.prefix_cache(16)
        miss = _device_prefill(m, cfg, ins(n))
        hit = _device_prefill(m, cfg, ins(n))
        for name, r in (("miss", miss), ("hit", hit)):
            for what, a, b in (("hidden", r[0], base[0]), ("logits", r[1], base[1])):
                err = float(np.abs(a - b).max())
                print(f"measured  {preset} n={n} {name} {what}: max |two-pass - one-pass| = {err:.3e}")
                assert np.isfinite(a).all() and np.allclose(a, b, rtol=1e-4, atol=1e-4), (name, what, err)
        np.testing.assert_array_equal(hit[0], miss[0])
        np.testing.assert_array_equal(hit[1], miss[1])
    finally:
        m.prefix_cache(16)


# ---------------------------------------------------------------- 4. odd cases
def test_an_fp32_entry_is_not_served_to_a_bf16_run(models):
    m, _, _ = _model(models, "tiny")
    try:
        m.set_kv_cache("fp32")
        m.prefix_cache(0)
        m.prefix_cache(16)
        assert _run(m, ins(7))[3][:2] == (0, 1)
        assert m.prefix_cache_bytes() == _entry_bytes(m, 7, "fp32")
        m.set_kv_cache("bf16")
        bf = _run(m, ins(7))
        assert bf[3][:2] == (0, 1)                             # computed again, in bf16
        assert m.prefix_cache_bytes() == _entry_bytes(m, 7, "bf16")   # the fp32 entry went with the dtype change
        assert _run(m, ins(7))[3][:2] == (1, 0)
        m.set_kv_cache("fp32")
        assert _run(m, ins(7))[3][:2] == (0, 1)
    finally:
        m.set_kv_cache("fp32")


def _gap(plan):
    plan[1][2] = 0          # rows 0 and 2 are prefix rows, row 1 is not


def _cid(plan):
    plan[1][1] = 5          # a prefix row with a codec id


def _late(plan):
    plan[-3][2] = 2         # a kind-2 row that is not among the leading rows


def _slot(plan):
    plan[1][4] = 5          # out of order


@pytest.mark.parametrize("spoil", [_gap, _cid, _late, _slot], ids=["gap", "cid", "late", "slot"])
def test_a_malformed_prefix_plan_is_refused(models, spoil):
    m, _, cfg = _model(models, "tiny")
    c0 = m.prefix_counters()
    assert _device_prefill(m, cfg, ins(4), malformed=spoil) == -1
    assert m.prefix_counters() == c0                           # nothing launched
    assert not isinstance(_device_prefill(m, cfg, ins(4)), int)   # the well-formed plan goes through


# ---------------------------------------------------------------- 5. queue
def test_queue_twice_second_run_has_no_miss(gpu, models):
    md = model_dir("tiny", eos_gain=manifest()["eos_gain"])
    m = qtts.QwenTTS(md)
    try:
        a, b = ins(12), ins(30, 40)
        per = [a, b, a, a, b, a, b]
        prompts = [IDS, prompt_ids("p128", 1300), prompt_ids("p128", 1301), IDS, prompt_ids("p128", 1310),
                   prompt_ids("p128", 1311), IDS]
        runs = []
        for _ in range(2):
            m.set_params(max_tokens=32, fixed=0, seed=7, **DEFAULT)
            c0 = m.prefix_counters()
            m.set_utterance_instruct(per)
            rc, audio = m.generate_queue(prompts, ["aiden"] * 7, ["english"] * 7, slots=3)
            assert rc == 0
            d = tuple(y - x for x, y in zip(c0, m.prefix_counters()))
            runs.append(([m.queue_codes(u) for u in range(7)], audio, d))
        assert runs[0][2][:2] == (5, 2), runs[0][2]            # two prefixes computed once, five admissions restored
        assert runs[1][2][:2] == (7, 0), runs[1][2]
        assert runs[0][2][2] - runs[1][2][2] == 12 + 30        # the second call sends the two prefixes' rows fewer
        for u in range(7):
            np.testing.assert_array_equal(runs[1][0][u], runs[0][0][u], err_msg=f"utterance {u}")
            np.testing.assert_array_equal(runs[1][1][u], runs[0][1][u], err_msg=f"utterance {u} audio")
    finally:
        m.close()
