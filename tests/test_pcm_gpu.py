"""The live audio front door as callers use it: ``artalk_amd.live_audio.LiveAudio`` (artalk_pcm_*) and the engine's audio half
(``open_stream(audio=...)``, ``stream_feed``, ``stream_audio_end``, ``stream_ready``, ``stream_step(streams)``).  Raw packets in, the
bits of the whole-clip path out: blocks equal ``resample_mean_16k`` of the whole signal cut into rows, and frames equal those of
yardstick streams on the same model that are stepped through the existing ``stream_step(streams, chunks, n_valid)``."""
import numpy as np
import pytest
import torch

from artalk_amd import live_audio
from artalk_amd.audio import resample_mean_16k
from audio_cases import make_signal
from conftest import get_gpu_model

pytestmark = pytest.mark.gpu

BLOCK = 640


def bits(t):
    return t.view(torch.int32)


def s16_signal(nch, n, seed):
    """(int16 (n, nch) interleaved, float32 (nch, n) = value / 32768 as read_wav gives it)"""
    q = np.clip(np.round(make_signal("noise", nch, n, seed) * 32768.0 / 1.5), -32768, 32767).astype("<i2")
    return np.ascontiguousarray(q.T), torch.from_numpy(q.astype(np.float32) / np.float32(32768.0))


def run_live(pcm, sr, nch, dtype, packet, as_packet, geometry):
    """Pushes ``pcm`` in packets of ``packet`` frames, takes whatever comes ready, ends, drains: (rows, n_valid) with the arithmetic checked
    at every step."""
    orig, nw, width = geometry
    live = live_audio.LiveAudio(block=BLOCK, ring_blocks=2)
    st = live.open(sr, channels=nch, dtype=dtype)
    n = pcm.shape[0]
    rows, valid, n_in, taken = [], [], 0, 0

    def check(ended):
        have = (live_audio.total_outputs(n_in, orig, nw) if ended else live_audio.emitted(n_in, orig, nw, width)) - taken
        assert live.available(st) == have and live.ended(st) == ended
        assert live.ready(st) == (have >= BLOCK or (ended and have >= 1))
        assert live.drained(st) == (ended and have == 0)
        return have

    check(False)
    for at in range(0, n, packet):
        pkt = pcm[at:at + packet]
        live.push([st], [as_packet(pkt)])
        n_in += pkt.shape[0]
        check(False)
        while live.ready(st):
            assert live.next_valid([st]) == [BLOCK]
            r, nv = live.take([st])
            assert r.shape == (1, BLOCK) and nv == [BLOCK]
            rows.append(r[0]); valid.append(nv[0]); taken += nv[0]
            check(False)
    with pytest.raises(RuntimeError):
        live.take([st])                                               # less than a block and not ended: refused, nothing taken
    check(False)
    live.end([st])
    while check(True):
        r, nv = live.take([st])
        rows.append(r[0]); valid.append(nv[0]); taken += nv[0]
    assert live.drained(st)
    with pytest.raises(RuntimeError):
        live.push([st], [as_packet(pcm[:1])])                         # a push after end
    st.close()
    with pytest.raises(ValueError):
        live.available(st)                                            # a closed id
    return torch.stack(rows), valid


def test_live_audio_rows_equal_the_offline_result_from_host_and_device_packets():
    """48 kHz stereo s16, 60 000 frames in 20 ms packets -> 20 000 samples = 31 rows of 640 and one of 160, through a ring of two rows."""
    pcm, x = s16_signal(2, 60000, 7)
    want = resample_mean_16k(x, 48000, "cuda")
    assert want.shape == (20000,)
    full = torch.zeros(32 * BLOCK, device="cuda")
    full[:20000] = want
    got = {}
    for kind, as_packet in (("bytes", lambda p: p.tobytes()), ("device", lambda p: torch.from_numpy(p.copy()).cuda())):
        rows, valid = run_live(pcm, 48000, 2, "s16", 960, as_packet, (3, 1, 19))
        assert valid == [BLOCK] * 31 + [160] and rows.shape == (32, BLOCK)
        assert torch.equal(bits(rows.reshape(-1)), bits(full)), kind   # (zero past the last row's 160 real samples)
        got[kind] = rows
    assert torch.equal(bits(got["bytes"]), bits(got["device"]))


@pytest.mark.parametrize("sr,nch,dtype,packet,geometry", [(44100, 1, "f32", 441, (441, 160, 17)), (16000, 3, "s16", 333, (1, 1, 0)),
                                                           (8000, 2, "f32", 97, (1, 2, 7))])
def test_live_audio_at_other_rates_and_formats(sr, nch, dtype, packet, geometry):
    n = 5 * sr // 16 + 13
    if dtype == "s16":
        pcm, x = s16_signal(nch, n, sr)
    else:
        x = torch.from_numpy(make_signal("noise", nch, n, sr))
        pcm = np.ascontiguousarray(x.numpy().T)
    if sr == 16000:      # the formula with one tap of 1.0: the channels summed in order, then divided
        want = torch.from_numpy((x[0] + x[1] + x[2]).numpy() / np.float32(3.0)).cuda()
    else:
        want = resample_mean_16k(x, sr, "cuda")
    kinds = [lambda p: p, lambda p: torch.from_numpy(p.copy()), lambda p: p.tobytes()]      # numpy, CPU tensor, bytes
    rows, valid = run_live(pcm, sr, nch, dtype, packet, kinds[nch - 1], geometry)
    assert sum(valid) == want.shape[0] and all(v == BLOCK for v in valid[:-1])
    flat = rows.reshape(-1)
    assert torch.equal(bits(flat[:want.shape[0]]), bits(want)) and not flat[want.shape[0]:].any()


def test_one_push_serves_streams_of_several_rates_and_refuses_whole():
    live = live_audio.LiveAudio(block=BLOCK, ring_blocks=2, max_streams=3)
    a, b, c = live.open(48000, 2, "s16"), live.open(44100, 1, "f32"), live.open(16000, 1, "s16")
    with pytest.raises(RuntimeError):
        live.open(8000)                                               # max_streams
    pa, xa = s16_signal(2, 3000, 1)
    xb = torch.from_numpy(make_signal("noise", 1, 2500, 2))
    pc, xc = s16_signal(1, 700, 3)
    for lo in range(0, 3000, 500):
        live.push([a, b, c], [pa[lo:lo + 500], xb[0, lo:lo + 500].numpy(), pc[lo:lo + 500].tobytes()])      # b and c run out: empty packets
    with pytest.raises(ValueError):
        live.push([a, a], [pa[:1], pa[:1]])
    with pytest.raises(ValueError):
        live.push([a], [pa[:10].astype(np.float32)])                  # another dtype than the stream's
    with pytest.raises(ValueError):
        live.push([a], [b"123"])                                      # no whole frame
    with pytest.raises(RuntimeError):
        live.push([c, a], [pc[:1], np.zeros((4000, 2), dtype="<i2")])  # a's 1333 samples do not fit 1280 - 993: c does not move either
    assert live.available(c) == 700
    live.end([a, b, c])
    for st, x, sr in ((a, xa, 48000), (b, xb, 44100), (c, xc, 16000)):
        want = resample_mean_16k(x, sr, "cuda")
        got = []
        while not live.drained(st):
            r, nv = live.take([st])
            got.append(r[0, :nv[0]])
        assert torch.equal(bits(torch.cat(got)), bits(want)), sr


# ---------------------------------------------------------------------------------------------- the engine
SPC = 64000


def test_engine_streams_fed_raw_packets_equal_streams_stepped_with_offline_chunks():
    from artalk_amd.engine import ARTAvatarInferEngine
    m = get_gpu_model("tiny")
    m.set_precision("f32")
    eng = ARTAvatarInferEngine(model=m)
    specs = [(48000, 2, "s16", 2.3), (44100, 1, "f32", 1.0), (16000, 1, "s16", 0.4)]
    try:
        pcm, offline = [], []
        for i, (sr, nch, dtype, blocks) in enumerate(specs):
            n = int(round(blocks * SPC * sr / 16000))
            if dtype == "s16":
                p, x = s16_signal(nch, n, 40 + i)
            else:
                x = torch.from_numpy(make_signal("noise", nch, n, 40 + i))
                p = np.ascontiguousarray(x.numpy().T)
            pcm.append(p)
            offline.append(resample_mean_16k(x, sr, "cuda"))
        assert [int(o.shape[0]) for o in offline] == [147200, 64000, 25600]
        live = [eng.open_stream(audio=(sr, nch, dtype)) for sr, nch, dtype, _ in specs]
        yard = [eng.open_stream() for _ in specs]
        with pytest.raises(ValueError):
            eng.stream_feed([yard[0]], [b""])                          # no audio half
        with pytest.raises(ValueError):
            eng.open_stream(audio=(44101, 1, "s16"))
        at, done_feeding, fed_blocks = [0, 0, 0], [False] * 3, [0, 0, 0]
        rec_live, rec_yard = [[] for _ in specs], [[] for _ in specs]
        steps, rounds = [], 0
        while not all(eng.stream_drained(st) for st in live):
            rounds += 1
            feed = [i for i in range(3) if not done_feeding[i]]
            if feed:      # one 20 ms packet of every stream that still has audio, in one call
                pk = []
                for i in feed:
                    k = specs[i][0] // 50
                    pk.append(pcm[i][at[i]:at[i] + k])
                    at[i] += k
                eng.stream_feed([live[i] for i in feed], pk)
                over = [i for i in feed if at[i] >= pcm[i].shape[0]]
                if over:
                    eng.stream_audio_end([live[i] for i in over])
                    for i in over:
                        done_feeding[i] = True
            ready = eng.stream_ready(live) if rounds % 4 == 2 else []      # (the loop looks every 80 ms: two streams come ready together)
            if not ready:
                continue
            idx = [live.index(st) for st in ready]
            frames, spans = eng.stream_step(ready, smooth=True)
            chunks = torch.zeros(len(idx), SPC, device="cuda")
            nv = []
            for r, i in enumerate(idx):
                seg = offline[i][fed_blocks[i] * SPC:(fed_blocks[i] + 1) * SPC]
                chunks[r, :seg.shape[0]] = seg
                nv.append(int(seg.shape[0]))
                fed_blocks[i] += 1
            y_frames, y_spans = eng.stream_step([yard[i] for i in idx], chunks, n_valid=nv, smooth=True)
            assert spans == y_spans and torch.equal(bits(frames), bits(y_frames)), f"step {len(steps)} of streams {idx}"
            for r, i in enumerate(idx):
                rec_live[i].append(frames[r, :spans[r][1]].clone())
            steps.append(idx)
        assert steps == [[2], [0, 1], [0], [0]]
        # the clip that ended on a block boundary was never told so: it is drained, not smoothed to its end, and a flush ends it
        assert [st.smooth_done for st in live] == [True, False, True] == [st.smooth_done for st in yard]
        tail, tspans = eng.stream_flush([live[1]])
        y_tail, y_tspans = eng.stream_flush([yard[1]])
        assert tspans == y_tspans == [(96, 4)] and torch.equal(bits(tail), bits(y_tail))
        assert [sum(int(f.shape[0]) for f in rec) for rec in rec_live] == [230, 96, 40]
        with pytest.raises(RuntimeError):
            eng.stream_step([live[0]], smooth=True)                    # drained: nothing to take
        # a stream that ends shorter than 9 frames: refused before its block leaves the ring
        short = eng.open_stream(audio=(16000, 1, "s16"))
        eng.stream_feed([short], [s16_signal(1, 4800, 9)[0]])
        assert eng.stream_ready([short]) == []
        eng.stream_audio_end([short])
        assert eng.stream_ready([short]) == [short]
        with pytest.raises(ValueError, match="window_length"):
            eng.stream_step([short], smooth=True)
        a = eng._audio_of([short])[0]
        assert eng.live_audio.available(a) == 4800 and short.steps == 0
        raw, nf = eng.stream_step([short])                             # without the smoother the same block goes through
        assert nf == [8] and raw.shape == (1, 100, 106) and eng.stream_drained(short)
        for st in live + yard + [short]:
            eng.close_stream(st)
        assert a.closed and all(st.closed for st in live)
    finally:
        m.close_sessions(list(m._sessions.values()))
        m.stream_end()
        m.set_precision("f32")
