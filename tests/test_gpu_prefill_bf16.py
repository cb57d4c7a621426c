"""The bf16 prefill precision through qwen_tts_set_prefill_precision and
qwen_tts_talker_prefill on the smallest synthetic talker the one-plane planner
covers: `tiny` with widths that are multiples of 256, two layers.  The hidden's
distance to exact is printed, not asserted: the mode's bar is the kernel bound
of test_gpu_pgemmh.py.  Measured on an MI355X, 40 rows: 2.2e-3 relative.
"""
import os

import numpy as np
import pytest

from conftest import MODEL_ROOT
from oracle_py import DEFAULT
from synth_model import ensure_model, prompt_ids

import qtts

pytestmark = pytest.mark.gpu

SMALL = dict(H=256, I=512, NH=4, KV=2, HD=64, mrope=[16, 8, 8])


@pytest.fixture(scope="module")
def md(gpu):
    return ensure_model(os.path.join(MODEL_ROOT, "tiny_w256"), "tiny", overrides=SMALL)


def _prefill(m, n):
    """(hidden, k_pgemmh launches of the call) of n seeded rows"""
    c0 = qtts.Kernels.pgemmh_launches()
    h = m.prefill((np.random.default_rng(n).standard_normal((n, m.cfg.talker_hidden)) * 0.5).astype(np.float32))
    return h, qtts.Kernels.pgemmh_launches() - c0


def test_switch_rows_and_determinism(md, monkeypatch):
    monkeypatch.delenv("QTTS_HIP_PREFILL", raising=False)
    plain, m = qtts.QwenTTS(md), qtts.QwenTTS(md)
    try:
        assert m.prefill_precision() == qtts.PREFILL_EXACT
        want = {n: _prefill(plain, n) for n in (12, 40)}       # a context that never called the setter
        assert all(moved == 0 for _, moved in want.values())
        m.set_prefill_precision("bf16")
        m.set_prefill_precision("exact")
        for n in (12, 40):                                     # switched off again
            h, moved = _prefill(m, n)
            assert moved == 0 and h.tobytes() == want[n][0].tobytes(), n
        m.set_prefill_precision("bf16")
        h, moved = _prefill(m, 12)                             # <= 16 rows: the exact kernels
        assert moved == 0 and h.tobytes() == want[12][0].tobytes()
        h, moved = _prefill(m, 40)
        assert moved == 4 * m.cfg.talker_layers, moved         # q|k|v, O, gate|up, down of every layer
        assert np.isfinite(h).all() and h.tobytes() != want[40][0].tobytes()
        assert _prefill(m, 40)[0].tobytes() == h.tobytes()
        e = want[40][0].astype(np.float64)
        print(f"measured  40 rows, hidden bf16 against exact: |d| / |exact| = "
              f"{np.linalg.norm(h - e) / np.linalg.norm(e):.3e}, max |d| = {np.abs(h - e).max():.3e}")
        with pytest.raises(ValueError):
            m.set_prefill_precision(2)
        assert m.prefill_precision() == qtts.PREFILL_BF16
    finally:
        plain.close()
        m.close()


def test_env_sets_the_default(md, monkeypatch):
    monkeypatch.setenv("QTTS_HIP_PREFILL", "bf16")
    m = qtts.QwenTTS(md)
    try:
        assert m.prefill_precision() == qtts.PREFILL_BF16
        assert _prefill(m, 40)[1] > 0
    finally:
        m.close()


def test_a_prefix_entry_is_served_only_in_its_own_mode(md, monkeypatch):
    monkeypatch.delenv("QTTS_HIP_PREFILL", raising=False)
    ins = np.random.default_rng(77).integers(1000, 100000, size=40).tolist()   # 40 prefix rows: the > 16-row path
    m = qtts.QwenTTS(md)

    def run():
        m.set_params(max_tokens=4096, fixed=2, seed=9, **DEFAULT)
        c0, p0 = m.prefix_counters(), qtts.Kernels.pgemmh_launches()
        m.set_utterance_instruct([ins])
        assert m.generate(prompt_ids("short"), "aiden", "english") is not None
        hits = tuple(b - a for a, b in zip(c0, m.prefix_counters()))[:2]
        return hits, qtts.Kernels.pgemmh_launches() - p0, m.last_codes()

    try:
        made = run()
        assert made[:2] == ((0, 1), 0)                         # computed in exact mode
        m.set_prefill_precision("bf16")
        other = run()
        assert other[0] == (0, 1) and other[1] > 0             # not served: computed again, on k_pgemmh
        again = run()
        assert again[:2] == ((1, 0), 0) and np.array_equal(again[2], other[2])   # its own entry is
        m.set_prefill_precision("exact")
        back = run()
        assert back[:2] == ((1, 0), 0) and np.array_equal(back[2], made[2])      # and the exact entry is still there
    finally:
        m.close()
