"""The ragged push of the multi-stream exact codec
(qwen_tts_codec_mstream_push_ragged): every stream of a push advances by its
own number of frames, still in one launch sequence per internal pass.  A pass
runs at the largest count left; a shorter stream's plane and stacked rows are
padded on the right, and the codec's causality keeps the padding out of every
valid column and out of the carried state.

Bounds are the multi-stream codec's (test_gpu_codec_mstream_pos.py): 1e-5
max-abs against the full decode of the same codes on the device, audio_close
(1e-4) against the oracle, and bit identity wherever two runs do the same
arithmetic.  The tiny codec's window is 72 (71 K/V rows kept) and a pass holds
16 frames.
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

    def _took(self, streams, counts, o):
        assert o is not None, (streams, counts, self.cur)
        for s, c, a in zip(streams, counts, o):
            assert len(a) == 1920 * c
            self.out[s].append(a)
            self.cur[s] += c
        assert [self.m.codec_mstream_pos(s) for s in streams] == [self.cur[s] for s in streams]

    def push(self, streams, T):
        c = np.stack([self.codes[s][self.cur[s]:self.cur[s] + T] for s in streams])
        assert c.shape[1] == T
        self._took(streams, [T] * len(streams), self.m.codec_mstream_push_any(streams, c))

    def ragged(self, streams, counts):
        cl = [self.codes[s][self.cur[s]:self.cur[s] + c] for s, c in zip(streams, counts)]
        assert [len(c) for c in cl] == list(counts)
        self._took(streams, counts, self.m.codec_mstream_push_ragged(streams, cl))

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


# ---------------------------------------------------------------- 1. equal counts: push_any, bit for bit
def test_equal_counts_are_push_any(tts_tiny):
    codes = list(codes_of(11, 3, sum(SCHED)))
    runs = []
    for ragged in (False, True):
        f = Feeder(tts_tiny, codes, 64)
        for T in SCHED:
            if ragged:
                f.ragged([0, 1, 2], [T, T, T])
            else:
                f.push([0, 1, 2], T)
        runs.append([f.audio(s) for s in range(3)])
    for s in range(3):
        np.testing.assert_array_equal(runs[0][s], runs[1][s])


# ---------------------------------------------------------------- 2. a ragged push is a prefix of the uniform one
def test_ragged_is_a_prefix_of_the_uniform_push(tts_tiny):
    m = tts_tiny
    codes = codes_of(12, 3, 16)              # (the uniform push: the same codes and 0 / 11 / 15 more)
    counts = [16, 5, 1]
    assert m.codec_mstream_begin(3, 32) == 0
    uni = m.codec_mstream_push_any([0, 1, 2], codes)
    assert uni is not None
    assert m.codec_mstream_begin(3, 32) == 0
    rag = m.codec_mstream_push_ragged([0, 1, 2], [codes[s][:counts[s]] for s in range(3)], counts=counts,
                                      ld_frames=16, fill=7.0)
    assert rag is not None
    assert [m.codec_mstream_pos(s) for s in range(3)] == counts
    for s in range(3):
        k = counts[s] * 1920
        np.testing.assert_array_equal(rag[s][:k], uni[s][:k])
        assert np.all(rag[s][k:] == 7.0)     # nothing past the stream's own samples


# ---------------------------------------------------------------- 3. the carried state after ragged pushes
START = [0, 60, 68]
RAGGED = [[1, 5, 16], [16, 5, 1], [23, 2, 16], [3, 16, 7]]
# [1, 5, 16]: stream 1 (60 rows) would cross row 71 with its padding (60 + 16) and does not with
#   its 5 frames: it must not shift; stream 2 (68 + 16) shifts
# [23, 2, 16]: two passes, streams 1 and 2 are no part of the second


def test_carried_state_after_ragged_pushes(tts_tiny, oracle):
    m = tts_tiny
    tot = [sum(r[s] for r in RAGGED) for s in range(3)]
    codes = [codes_of(20 + s, 1, START[s] + tot[s])[0] for s in range(3)]
    f = Feeder(m, codes, 160)
    f.push([1], START[1])
    f.push([2], START[2])
    for r in RAGGED:
        f.ragged([0, 1, 2], r)               # (checks codec_mstream_pos against the running sums)
    assert f.cur == [START[s] + tot[s] for s in range(3)] == [43, 88, 108]
    assert _worst(m, f, range(3), "ragged pushes from 0 / 60 / 68") < 1e-5
    for s in range(3):
        audio_close(f.audio(s), oracle.codec_decode(f.codes[s]))


# ---------------------------------------------------------------- 4. no crosstalk across counts
def test_a_stream_does_not_see_its_neighbours_counts(tts_tiny):
    m = tts_tiny
    codes = list(codes_of(30, 3, 16))
    runs = []
    for counts in ([16, 16, 16], [16, 1, 5]):
        f = Feeder(m, codes, 32)
        f.ragged([0, 1, 2], counts)
        runs.append(f.audio(0))
    np.testing.assert_array_equal(runs[0], runs[1])


# ---------------------------------------------------------------- 5. more than 16 streams (the wide grouping)
def test_seventeen_streams_with_ragged_counts(tts_tiny):
    m = tts_tiny
    n = 17
    start = [5 * s % 90 for s in range(n)]
    counts = [s % 16 + 1 for s in range(n)]
    codes = [codes_of(50 + s, 1, start[s] + counts[s])[0] for s in range(n)]
    f = Feeder(m, codes, 128)
    for s in range(n):
        if start[s]:
            f.push([s], start[s])
    f.ragged(list(range(n)), counts)
    assert f.cur == [start[s] + counts[s] for s in range(n)]
    assert _worst(m, f, range(n), "17 streams, counts s mod 16 + 1 at 5 s mod 90") < 1e-5


# ---------------------------------------------------------------- 6. refusals
def _raw_ragged(m, streams, counts, ld=4):
    """the push as given (no checks on this side): the return value"""
    st = np.ascontiguousarray(streams, np.int32)
    n = len(st)
    codes = np.zeros((n, ld, 16), np.int32)
    outs = [np.full(ld * 1920, 7.0, np.float32) for _ in range(n)]
    po = (_fp * n)(*[o.ctypes.data_as(_fp) for o in outs])
    cn = None if counts is None else np.ascontiguousarray(counts, np.int32)
    rc = qtts.lib().qwen_tts_codec_mstream_push_ragged(m.ctx, n, st.ctypes.data_as(_ip), codes.ctypes.data_as(_ip),
                                                       None if cn is None else cn.ctypes.data_as(_ip), ld, po)
    if rc < 0:
        assert all(np.all(o == 7.0) for o in outs)      # nothing was written
    return rc


def test_refusals_leave_the_streams_untouched(tts_tiny, capfd):
    m = tts_tiny
    codes = list(codes_of(60, 3, 16))

    def sequence(disturb):
        f = Feeder(m, codes, 16)
        f.ragged([0, 1, 2], [2, 6, 2])                            # positions 2, 6, 2
        if disturb:
            assert _raw_ragged(m, [0, 1, 2], None) == -1          # no counts
            assert _raw_ragged(m, [0, 1, 2], [1, 0, 1]) == -1     # a count < 1
            assert _raw_ragged(m, [0, 1, 2], [1, 1, -2]) == -1
            assert _raw_ragged(m, [0, 1, 2], [1, 5, 1]) == -1     # a count above ld_frames (4)
            assert _raw_ragged(m, [0, 1, 1], [1, 1, 1]) == -1     # (push_any's: listed twice)
            capfd.readouterr()
            assert _raw_ragged(m, [0, 1, 2], [11, 11, 11], ld=11) == -1   # only stream 1 would pass 16 (6 + 11)
            assert "stream 1:" in capfd.readouterr().err
            assert [m.codec_mstream_pos(s) for s in range(3)] == [2, 6, 2]
        f.ragged([0, 1, 2], [4, 10, 1])                           # 6, 16, 3: stream 1 exactly to max_frames
        if disturb:
            capfd.readouterr()
            assert _raw_ragged(m, [0, 1], [2, 1]) == -1           # stream 1 is full
            assert "stream 1:" in capfd.readouterr().err
        f.ragged([2, 0], [13, 10])
        assert f.cur == [16, 16, 16]
        return [f.audio(s) for s in range(3)]

    clean = sequence(False)
    disturbed = sequence(True)
    for x, y in zip(clean, disturbed):
        np.testing.assert_array_equal(x, y)
