"""The multi-stream exact codec with its streams at independent positions
(qwen_tts_codec_mstream_push_any, qwen_tts_codec_mstream_reset): one launch
sequence per push, every stacked row rotated, cached and windowed by its own
stream's position.

Bounds are the multi-stream codec's (test_gpu_codec_mstream.py): 1e-5 max-abs
against the full decode of the same codes on the device, audio_close (1e-4)
against the oracle, and bit identity wherever two runs do the same arithmetic.
The tiny codec's window is 72 (71 K/V rows kept) and a pass holds 16 frames, so
positions 0, 60 and 75 put a stream that never shifts, one that crosses the
window edge and one whose window is full into the same launches.
"""
import ctypes as C

import numpy as np
import pytest

import qtts

pytestmark = pytest.mark.gpu

_ip, _fp = C.POINTER(C.c_int), C.POINTER(C.c_float)
SCHED = [1, 3, 7, 16, 23]        # (23: two passes in one push)


def audio_close(a, ref):
    assert a is not None and a.shape == ref.shape, (None if a is None else a.shape, ref.shape)
    mse = float(np.mean((a.astype(np.float64) - ref) ** 2)) if len(ref) else 0.0
    assert mse < 1e-4, mse
    if len(ref):
        assert np.abs(a - ref).max() < 1e-4, np.abs(a - ref).max()


_CODES, _FULL = {}, {}


def codes_of(seed, n, T):
    """[n, T, 16] random codes, fixed per (seed, n, T)"""
    if (seed, n, T) not in _CODES:
        c = np.random.default_rng(seed).integers(0, 2048, size=(n, T, 16)).astype(np.int32)
        c.setflags(write=False)
        _CODES[(seed, n, T)] = c
    return _CODES[(seed, n, T)]


def full_decode(m, codes):
    """codec_decode of one stream's codes, computed once per code array"""
    key = codes.tobytes()
    if key not in _FULL:
        a = m.codec_decode(np.ascontiguousarray(codes))
        a.setflags(write=False)
        _FULL[key] = a
    return _FULL[key]


class Feeder:
    """n streams fed from codes[s] (arrays of their own lengths), each from its own cursor"""

    def __init__(self, m, codes, max_frames):
        self.m, self.codes = m, codes
        self.cur = [0] * len(codes)
        self.out = [[] for _ in codes]
        assert m.codec_mstream_begin(len(codes), max_frames) == 0

    def push(self, streams, T, any_position=True):
        c = np.stack([self.codes[s][self.cur[s]:self.cur[s] + T] for s in streams])
        assert c.shape[1] == T
        o = self.m.codec_mstream_push(streams, c, any_position=any_position)
        assert o is not None, (streams, T, self.cur)
        for s, a in zip(streams, o):
            assert len(a) == 1920 * T
            self.out[s].append(a)
            self.cur[s] += T
        assert [self.m.codec_mstream_pos(s) for s in streams] == [self.cur[s] for s in streams]

    def audio(self, s):
        return np.concatenate(self.out[s])


def _worst(m, f, streams, what):
    worst = 0.0
    for s in streams:
        got, full = f.audio(s), full_decode(m, f.codes[s][:f.cur[s]])
        assert got.shape == full.shape, (what, s)
        worst = max(worst, float(np.abs(got - full).max()))
    print(f"measured  {what}: largest |stream - full decode| {worst:.3e}")
    return worst


# ---------------------------------------------------------------- 1. equal positions: the older push, bit for bit
def test_equal_positions_are_the_same_position_push(tts_tiny):
    codes = list(codes_of(11, 3, sum(SCHED)))
    runs = []
    for any_position in (False, True):
        f = Feeder(tts_tiny, codes, 64)
        for T in SCHED:
            f.push([0, 1, 2], T, any_position=any_position)
        runs.append([f.audio(s) for s in range(3)])
    for s in range(3):
        np.testing.assert_array_equal(runs[0][s], runs[1][s])


# ---------------------------------------------------------------- 2. mixed positions against the full decode
START = [0, 60, 75]


def _mixed_codes():
    return [codes_of(20 + s, 1, START[s] + sum(SCHED))[0] for s in range(3)]


@pytest.fixture(scope="module")
def mixed(tts_tiny):
    """stream 0 at 0, stream 1 advanced alone by 60 frames, stream 2 by 75; then SCHED for all three together"""
    f = Feeder(tts_tiny, _mixed_codes(), 160)
    f.push([1], START[1], any_position=False)
    f.push([2], START[2], any_position=False)
    for T in SCHED:
        f.push([0, 1, 2], T)
    return f


def test_mixed_positions_equal_the_full_decodes(tts_tiny, oracle, mixed):
    assert mixed.cur == [50, 110, 125]
    assert _worst(tts_tiny, mixed, range(3), "positions 0 / 60 / 75") < 1e-5
    for s in range(3):
        audio_close(mixed.audio(s), oracle.codec_decode(mixed.codes[s]))


# ---------------------------------------------------------------- 3. no crosstalk across positions
def test_a_stream_does_not_see_where_its_neighbours_are(tts_tiny, mixed):
    other = [_mixed_codes()[0], codes_of(31, 1, 50)[0], codes_of(32, 1, 50)[0]]
    f = Feeder(tts_tiny, other, 160)
    for T in SCHED:
        f.push([0, 1, 2], T)
    np.testing.assert_array_equal(f.audio(0), mixed.audio(0))
    assert not np.array_equal(f.audio(1), mixed.audio(1)[-50 * 1920:])


# ---------------------------------------------------------------- 4. reset of one stream
def test_reset_restarts_one_stream_and_leaves_the_others(tts_tiny):
    m = tts_tiny
    base = codes_of(40, 3, 100)
    fresh = codes_of(41, 1, 20)[0]

    def run(reset):
        # stream 1: its first 80 frames, then `fresh` (after a reset: from position 0)
        codes = [base[0], np.concatenate([base[1, :80], fresh]), base[2]]
        f = Feeder(m, codes, 128)
        for T in (16, 64):
            f.push([0, 1, 2], T)
        if reset:
            assert m.codec_mstream_reset(1) == 0
            assert [m.codec_mstream_pos(s) for s in range(3)] == [80, 0, 80]
            f.codes[1] = fresh
            f.cur[1] = 0
            f.out[1] = []
        for T in (4, 16):
            f.push([0, 1, 2], T)
        return f

    a, b = run(True), run(False)
    assert a.cur == [100, 20, 100] and b.cur == [100, 100, 100]
    assert _worst(m, a, [1], "the reset stream's 20 new frames") < 1e-5
    assert _worst(m, a, [0, 2], "its neighbours' 100 frames") < 1e-5
    for s in (0, 2):
        np.testing.assert_array_equal(a.audio(s), b.audio(s))
    assert not np.array_equal(a.audio(1), b.audio(1)[-20 * 1920:])


# ---------------------------------------------------------------- 5. more than 16 streams (the wide grouping)
def test_seventeen_streams_at_scattered_positions(tts_tiny):
    m = tts_tiny
    n, sched = 17, [1, 4, 16]
    start = [5 * s % 90 for s in range(n)]
    codes = [codes_of(50 + s, 1, start[s] + sum(sched))[0] for s in range(n)]
    f = Feeder(m, codes, 128)
    for s in range(n):
        if start[s]:
            f.push([s], start[s], any_position=False)
    for T in sched:
        f.push(list(range(n)), T)
    assert f.cur == [start[s] + sum(sched) for s in range(n)]
    assert _worst(m, f, range(n), "17 streams at 5 s mod 90") < 1e-5


# ---------------------------------------------------------------- 6. refusals
def _raw_push(m, streams, T, n=None, any_position=True):
    """the push as given (no checks on this side): the return value"""
    st = np.asarray(streams, np.int32)
    n = len(st) if n is None else n
    k = max(len(st), 1)
    st = np.ascontiguousarray(np.resize(st, k) if len(st) else np.zeros(1, np.int32))
    codes = np.zeros((k, max(T, 1), 16), np.int32)
    outs = [np.full(max(T, 1) * 1920, 7.0, np.float32) for _ in range(k)]
    po = (_fp * k)(*[o.ctypes.data_as(_fp) for o in outs])
    fn = qtts.lib().qwen_tts_codec_mstream_push_any if any_position else qtts.lib().qwen_tts_codec_mstream_push
    rc = fn(m.ctx, n, st.ctypes.data_as(_ip), codes.ctypes.data_as(_ip), T, po)
    if rc < 0:
        assert all(np.all(o == 7.0) for o in outs)      # nothing was written
    return rc


def test_refusals_leave_the_streams_untouched(tts_tiny, tiny_dir, capfd):
    m = tts_tiny
    codes = list(codes_of(60, 3, 16))

    def sequence(disturb):
        f = Feeder(m, codes, 16)
        f.push([0, 1, 2], 2)
        if disturb:
            assert _raw_push(m, [], 1, n=0) == -1                 # bad n
            assert _raw_push(m, [0, 1, 2, 0], 1, n=4) == -1       # more streams than begun
            assert _raw_push(m, [0, 3], 1) == -1                  # index out of range
            assert _raw_push(m, [-1], 1) == -1
            assert _raw_push(m, [1, 1], 1) == -1                  # listed twice
            assert _raw_push(m, [0, 1], 0) == -1                  # T < 1
            assert _raw_push(m, [0, 1], -3) == -1
        f.push([1], 4)                                            # positions 2, 6, 2
        if disturb:
            capfd.readouterr()
            assert _raw_push(m, [0, 1, 2], 11) == -1              # only stream 1 would pass 16 (6 + 11)
            assert "stream 1:" in capfd.readouterr().err
            assert _raw_push(m, [0, 1], 1, any_position=False) == -1      # the older push: positions 2 and 6
            assert m.codec_mstream_reset(-1) == -1
            assert m.codec_mstream_reset(3) == -1
            assert [m.codec_mstream_pos(s) for s in range(3)] == [2, 6, 2]
        f.push([0, 1, 2], 4)                                      # 6, 10, 6
        f.push([0, 2, 1], 6)                                      # 12, 16, 12: stream 1 exactly to max_frames
        if disturb:
            assert _raw_push(m, [0, 1], 1) == -1                  # stream 1 is full
            assert _raw_push(m, [1], 1) == -1
        f.push([0, 2], 4)
        assert f.cur == [16, 16, 16]
        return [f.audio(s) for s in range(3)]

    clean = sequence(False)
    disturbed = sequence(True)
    for x, y in zip(clean, disturbed):
        np.testing.assert_array_equal(x, y)
    # a context that never began a multi-stream
    fresh = qtts.QwenTTS(tiny_dir)
    try:
        assert fresh.codec_mstream_reset(0) == -1
        assert _raw_push(fresh, [0], 1) == -1
        assert fresh.codec_mstream_pos(0) == -1
    finally:
        fresh.close()
