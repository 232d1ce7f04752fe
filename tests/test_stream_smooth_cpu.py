"""The streaming Savitzky-Golay smoother (artalk_session_smooth, savgol_stream_kernel): the parts that need no GPU - the emission
arithmetic (model.smooth_span, mirrored by the library) and every refusal, each of which is made before the device is touched."""
import ctypes as C

import pytest

from artalk_amd import capi
from artalk_amd.model import smooth_span

P = 4096      # a 16-byte aligned address that is never dereferenced: the checks come first
RAW, OUT = 100 * 106, 104 * 106


def brute_span(seen, nf, last):
    """Frames that are final after this call and were not before: t is final once frames t + 1 .. t + 4 exist, or the stream has ended."""
    total = seen + nf
    final_before = {t for t in range(seen) if t + 4 < seen}
    final_now = {t for t in range(total) if last or t + 4 < total}
    new = sorted(final_now - final_before)
    if not new:
        return max(0, seen - 4), 0
    assert new == list(range(new[0], new[0] + len(new)))
    return new[0], len(new)


@pytest.mark.parametrize("k", range(4))
def test_spans_tile_the_stream_exactly_once(k):
    for v in range(101):
        seen, covered = 0, []
        schedule = [(100, False)] * k + [(v, True)]
        if seen + 100 * k + v == 0:
            continue
        for nf, last in schedule:
            first, count = smooth_span(seen, nf, last)
            assert (first, count) == brute_span(seen, nf, last), (k, v, seen)
            assert 0 <= count <= 104
            covered += list(range(first, first + count))
            seen += nf
        assert covered == list(range(seen)), (k, v)


def test_first_step_emits_96_then_100():
    assert smooth_span(0, 100, False) == (0, 96)
    assert smooth_span(100, 100, False) == (96, 100)
    assert smooth_span(200, 100, True) == (196, 104)
    assert smooth_span(200, 0, True) == (196, 4)
    assert smooth_span(0, 9, True) == (0, 9)


def i32s(v):
    return (C.c_int32 * len(v))(*v)


def u8s(v):
    return (C.c_uint8 * len(v))(*v)


def i64s(v):
    return (C.c_int64 * max(len(v), 1))(*v)


def op(seen, nf, last, slots=P, raw=P, raw_stride=RAW + 22, out=P, out_stride=OUT, n=None):
    return capi.lib().artalk_op_savgol_stream(slots, raw, raw_stride, i32s(seen), i32s(nf), u8s(last), out, out_stride,
                                              len(seen) if n is None else n, None)


@pytest.fixture
def dry_run():
    L = capi.lib()
    L.artalk_op_rows_dry_run(1)
    yield
    L.artalk_op_rows_dry_run(0)


def test_op_is_exported_and_accepts_valid_rows(dry_run):
    L = capi.lib()
    for name in ("artalk_session_smooth", "artalk_op_savgol_stream", "artalk_op_session_smooth_check"):
        assert name in capi.SYMBOLS and hasattr(L, name), name
    assert op([0, 100, 200], [100, 100, 57], [0, 0, 1]) == capi.OK
    assert op([0], [9], [1]) == capi.OK                              # the minimum
    assert op([200], [0], [1], raw=None) == capi.OK                  # the flush reads no raw row
    assert op([100], [100], [1], raw_stride=RAW) == capi.OK


def test_op_refusals_come_before_the_device():
    for bad in (-1, 101, 1000):
        assert op([0], [bad], [1]) == capi.EINVAL                    # n_frames outside 0..100
    for short in (0, 1, 99):
        assert op([100], [short], [0]) == capi.EINVAL                # fewer than 100 frames without `last`
    assert op([0], [8], [1]) == capi.EINVAL                          # a stream that ends below 9 frames
    assert op([0], [0], [1]) == capi.EINVAL
    assert op([4], [4], [1]) == capi.EINVAL
    assert op([-1], [100], [0]) == capi.EINVAL
    assert op([2 ** 31 - 50], [100], [0]) == capi.EINVAL
    assert op([0], [100], [0], raw_stride=RAW - 1) == capi.EINVAL    # strides
    assert op([0], [100], [0], out_stride=OUT - 1) == capi.EINVAL
    assert op([0], [100], [0], out_stride=RAW) == capi.EINVAL
    assert op([0, 100], [100, 101], [0, 0]) == capi.EINVAL           # one bad row spoils the call
    assert op([0], [100], [0], n=0) == capi.EINVAL
    assert op([0], [100], [0], n=-3) == capi.EINVAL
    for null in ("slots", "raw", "out"):
        assert op([0], [100], [0], **{null: None}) == capi.EINVAL, null
    L = capi.lib()
    assert L.artalk_op_savgol_stream(P, P, RAW, None, i32s([100]), u8s([0]), P, OUT, 1, None) == capi.EINVAL
    assert L.artalk_op_savgol_stream(P, P, RAW, i32s([0]), None, u8s([0]), P, OUT, 1, None) == capi.EINVAL
    assert L.artalk_op_savgol_stream(P, P, RAW, i32s([0]), i32s([100]), None, P, OUT, 1, None) == capi.EINVAL


def check(ids, nf, last, open_=((7, 0, 0), (8, 100, 0), (9, 200, 1)), ended=(5,), raw_stride=RAW, out_stride=OUT, have_raw=1):
    """artalk_session_smooth's checks on a made-up session table: open sessions (id, frames seen, finished), ids a scale change closed."""
    n = len(ids)
    first, count = (C.c_int32 * max(n, 1))(), (C.c_int32 * max(n, 1))()
    msg = C.create_string_buffer(256)
    rc = capi.lib().artalk_op_session_smooth_check(
        i64s([o[0] for o in open_]), i64s([o[1] for o in open_]), u8s([o[2] for o in open_]), len(open_), i64s(list(ended)), len(ended),
        i64s(ids), n, have_raw, raw_stride, i32s(nf) if nf is not None else None, u8s(last) if last is not None else None, out_stride,
        first, count, msg, 256)
    return rc, msg.value.decode(), [(first[i], count[i]) for i in range(n)]


def test_session_smooth_accepts_and_reports_spans():
    rc, msg, spans = check([8, 7], [100, 100], [0, 0])
    assert rc == capi.OK and msg == "" and spans == [(96, 100), (0, 96)]
    rc, _, spans = check([8, 7], None, None)                         # NULL n_frames / last: 100 frames, not last
    assert rc == capi.OK and spans == [(96, 100), (0, 96)]
    rc, _, spans = check([8], [0], [1], have_raw=0)                  # the flush needs no raw frames
    assert rc == capi.OK and spans == [(96, 4)]
    rc, _, spans = check([7, 8], [9, 57], [1, 1])
    assert rc == capi.OK and spans == [(0, 9), (96, 61)]


def test_session_smooth_refusals_in_the_listed_order():
    rc, msg, _ = check([7, 6], [100, 100], [0, 0])
    assert rc == capi.EINVAL and "6 is not an open session" in msg   # unknown id
    rc, msg, _ = check([7, 8, 7], [100] * 3, [0] * 3)
    assert rc == capi.EINVAL and "listed twice" in msg               # duplicate id
    rc, msg, _ = check([7, 5], [100, 100], [0, 0])
    assert rc == capi.ESTATE and "the site scales changed since artalk_session_open" in msg
    for bad in (-1, 101):
        rc, msg, _ = check([7], [bad], [1])
        assert rc == capi.EINVAL and "outside 0..100" in msg
    rc, msg, _ = check([8], [99], [0])
    assert rc == capi.EINVAL and "without `last`" in msg
    rc, msg, _ = check([9], [100], [0])
    assert rc == capi.ESTATE and "smoothed to its end" in msg        # the smoother has finished
    rc, msg, _ = check([9], [0], [1])
    assert rc == capi.ESTATE                                         # a second flush
    rc, msg, _ = check([7], [8], [1])
    assert rc == capi.EINVAL and "window_length" in msg              # scipy's wording, as artalk_savgol
    rc, msg, _ = check([7], [0], [1])
    assert rc == capi.EINVAL and "window_length" in msg
    rc, msg, _ = check([7], [100], [0], raw_stride=RAW - 1)
    assert rc == capi.EINVAL and "raw_stride" in msg
    rc, msg, _ = check([7], [100], [0], out_stride=OUT - 1)
    assert rc == capi.EINVAL and "out_stride" in msg
    rc, msg, _ = check([7], [100], [0], have_raw=0)
    assert rc == capi.EINVAL and "no raw frames" in msg
    # a range error outranks the finished flag, the finished flag outranks the length
    rc, _, _ = check([9], [101], [1])
    assert rc == capi.EINVAL
    rc, _, _ = check([9], [50], [0])
    assert rc == capi.EINVAL
    rc, _, _ = check([7, 8], [100, 100], [0, 0], open_=())
    assert rc == capi.EINVAL
