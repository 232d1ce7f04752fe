"""``artalk_op_pcm_push`` / ``artalk_op_pcm_take`` (pcm_push_kernel, pcm_take_kernel of csrc/pcm.hip), one launch each, on the caller's own
buffers.  A stream's ring, its two carry buffers and its packet live in one block of NaN with guard bands of ``audio_cases.GUARD``
words between and around them; before every launch what it is going to write is NaN as well, afterwards every other word of the
block has its bits, the written ones are finite, and a second launch gives the same bits.  The 16 kHz samples of a chain of launches
over a signal cut into packets are bit-equal to ONE ``artalk_op_resample_mean`` launch on the whole signal - the whole-clip kernel
is the yardstick, nothing is allowed."""
import ctypes as C

import numpy as np
import pytest
import torch

from artalk_amd import capi, live_audio
from audio_cases import GUARD, RATIOS, make_signal, taps

pytestmark = pytest.mark.gpu

ONE = np.ones((1, 1), dtype=np.float32)      # 16 kHz in: the channel mean alone
GEOM = {"3:1": ("ta48000",) + tuple(RATIOS["ta48000"][2:5]), "441:160": ("ta44100",) + tuple(RATIOS["ta44100"][2:5]),
        "1:2": ("ta8000",) + tuple(RATIOS["ta8000"][2:5]), "1:1": (None, 1, 1, 0)}


def geometry(name):
    ratio, orig, nw, width = GEOM[name]
    return (taps(ratio) if ratio else ONE), orig, nw, width


def bits(t):
    return t.view(torch.int32)


def pcm_signal(fmt, nch, n, seed):
    """(interleaved samples (n, nch) as the sender has them, float32 (nch, n) as read_wav would hand them to the whole-clip kernel)"""
    x = make_signal("noise", nch, n, seed)
    if fmt == "f32":
        return np.ascontiguousarray(x.T), x
    q = np.clip(np.round(x * 32768.0 / 1.5), -32768, 32767).astype("<i2")
    return np.ascontiguousarray(q.T), (q.astype(np.float32) / np.float32(32768.0))


def whole_clip(name, x):
    """One launch of the whole-clip kernel on (nch, n) float32: the yardstick."""
    tp, orig, nw, width = geometry(name)
    nch, n = x.shape
    n_out = -((-n * nw) // orig)
    xd, td = torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(np.array(tp)).cuda()
    out = torch.full((n_out,), float("nan"), dtype=torch.float32, device="cuda")
    rc = capi.lib().artalk_op_resample_mean(capi.ptr(xd), nch, n, capi.ptr(td), orig, nw, width, capi.ptr(out), n_out, capi.current_stream_ptr())
    torch.cuda.synchronize()
    assert rc == capi.OK and torch.isfinite(out).all()
    return out


class Lane:
    """One stream on buffers of the test's own: [guard | ring | guard | carry 0 | guard | carry 1 | guard | packet | guard], float32 words."""

    def __init__(self, name, nch, fmt, ring_cap, max_frames, ring_start=0, misalign=0):
        self.tp, self.orig, self.nw, self.width = geometry(name)
        self.ntaps = 2 * self.width + self.orig
        self.nch, self.fmt, self.cap, self.misalign = nch, fmt, ring_cap, misalign
        self.eb = 2 if fmt == "s16" else 4
        self.stride = max(self.ntaps - 1, 1)                       # the tightest the carry can be
        cw = nch * self.stride
        pw = (max_frames * nch * self.eb + misalign + 3) // 4 + 4
        self.at = {}
        off = GUARD
        for key, words in (("ring", ring_cap), ("carry0", cw), ("carry1", cw), ("packet", pw)):
            off = (off + 3) & ~3                                    # every part starts on a 16-byte boundary
            self.at[key] = (off, words)
            off += words + GUARD
        self.arena = torch.full((off,), float("nan"), dtype=torch.float32, device="cuda")
        assert self.arena.data_ptr() % 16 == 0
        self.taps_dev = torch.from_numpy(np.array(self.tp)).cuda()
        self.taps_bits = bits(self.taps_dev).clone()
        self.n_in, self.written, self.cur = 0, ring_start, 0
        self.outs = []

    def addr(self, key, byte_off=0):
        return self.arena.data_ptr() + 4 * self.at[key][0] + byte_off

    def desc(self, pkt, end=False):
        """Writes the packet into its place and returns (descriptor, words the launch may write)."""
        frames = 0 if end else pkt.shape[0]
        q = live_audio.plan(self.n_in, frames, end, self.orig, self.nw, self.width)
        p0, pw = self.at["packet"]
        self.arena[p0:p0 + pw] = float("nan")
        if frames:
            raw = torch.from_numpy(np.frombuffer(pkt.tobytes(), dtype=np.uint8).copy()).cuda()
            lo = 4 * p0 + self.misalign
            self.arena.view(torch.uint8)[lo:lo + raw.numel()] = raw
        d = capi.PcmDesc(taps=self.taps_dev.data_ptr(), data=self.addr("packet", self.misalign) if frames else None,
                         carry_in=self.addr(f"carry{self.cur}"), carry_out=self.addr(f"carry{self.cur ^ 1}"), ring=self.addr("ring"),
                         orig=self.orig, nw=self.nw, width=self.width, nch=self.nch, format=capi.PCM_S16 if self.fmt == "s16" else capi.PCM_F32,
                         frames=frames, lead=q["lead"], carry_n=q["carry_n"], carry_from=q["carry_from"], carry_out_n=q["carry_out_n"],
                         carry_stride=self.stride, ring_cap=self.cap, ring_pos=self.written % self.cap, n_out=q["n_out"])
        ring_idx = (self.written + torch.arange(q["n_out"], device="cuda")) % self.cap + self.at["ring"][0]
        c0 = self.at[f"carry{self.cur ^ 1}"][0]
        carry_idx = (c0 + torch.arange(self.nch, device="cuda")[:, None] * self.stride + torch.arange(q["carry_out_n"], device="cuda")[None]).reshape(-1)
        self.q, self.ring_idx = q, ring_idx
        return d, torch.cat([ring_idx, carry_idx])

    def advance(self, frames, end=False):
        self.outs.append(self.arena[self.ring_idx].clone())
        self.n_in += frames
        self.written += self.q["n_out"]
        self.cur ^= 1


def launch(lanes, packets, end=False):
    """ONE launch for the listed lanes (a packet each, or the end), with the hygiene checks around it."""
    L = capi.lib()
    n = len(lanes)
    descs = (capi.PcmDesc * n)()
    may = []
    for i, (ln, pkt) in enumerate(zip(lanes, packets)):
        descs[i], w = ln.desc(pkt, end)
        may.append(w)
    table = torch.zeros(n * C.sizeof(capi.PcmDesc), dtype=torch.uint8, device="cuda")
    runs = []
    for _ in range(2):
        before = []
        for ln, w in zip(lanes, may):
            ln.arena[w] = float("nan")                                # ring span and carry out: NaN before the launch
            before.append(bits(ln.arena).clone())
        rc = L.artalk_op_pcm_push(descs, n, capi.ptr(table), table.numel(), capi.current_stream_ptr())
        assert rc == capi.OK, L.artalk_pcm_last_error(None)
        torch.cuda.synchronize()
        after = []
        for ln, w, b in zip(lanes, may, before):
            a = bits(ln.arena).clone()
            changed = a != b
            allowed = torch.zeros_like(changed)
            allowed[w] = True
            assert not (changed & ~allowed).any(), "a guard band, an input or a word of the ring outside the launch's span was written"
            assert torch.isfinite(ln.arena[w]).all(), f"{int((~torch.isfinite(ln.arena[w])).sum())} words are unwritten or not finite"
            assert torch.equal(bits(ln.taps_dev), ln.taps_bits), "the tap table was written"
            after.append(a)
        runs.append(after)
    for a, b in zip(*runs):
        assert torch.equal(a, b), "a second launch gives other bits"
    for ln, pkt in zip(lanes, packets):
        ln.advance(0 if end else pkt.shape[0], end)


def run_chain(name, nch, fmt, n, sizes, ring_cap, seed, ring_start=0, misalign=0):
    pcm, x = pcm_signal(fmt, nch, n, seed)
    ln = Lane(name, nch, fmt, ring_cap, max(sizes), ring_start, misalign)
    at = 0
    for s in sizes:
        launch([ln], [pcm[at:at + s]])
        at += s
    assert at == n
    launch([ln], [None], end=True)
    got = torch.cat(ln.outs)
    want = whole_clip(name, x)
    assert got.shape == want.shape
    bad = torch.nonzero(bits(got) != bits(want)).flatten()
    assert bad.numel() == 0, f"{bad.numel()} of {want.numel()} samples differ from the whole-clip kernel's, first at {bad[:4].tolist()}"


def split(n, size):
    return [size] * (n // size) + ([n % size] if n % size else [])


FORMS = [(1, "s16"), (2, "f32"), (3, "s16"), (1, "f32"), (2, "s16"), (3, "f32")]
RING = 600


def _cases():
    out = [("3:1", 1, "s16", 300, "1", 0)]
    for ri, name in enumerate(GEOM):
        _, orig, nw, width = GEOM[name]
        ntaps = 2 * width + orig
        n = {"3:1": 2999, "441:160": 3001, "1:2": 1201, "1:1": 2003}[name]
        half = -(-(RING // 2 + 1) * orig // nw) + orig                  # frames that emit more than half the ring
        for mi, mode in enumerate(("7", "97", str(orig), str(max(1, ntaps - 2)), str(half))):
            nch, fmt = FORMS[(ri + mi) % len(FORMS)]
            m = min(n, 300 * int(mode))      # (a launch a packet: at most 300 of them, so 300 frames for packets of one)
            if (name, mode) not in {(c[0], c[4]) for c in out}:
                out.append((name, nch, fmt, m, mode, ri + mi))
    return out


@pytest.mark.parametrize("name,nch,fmt,n,size,k", _cases())
def test_a_chain_of_pushes_equals_one_whole_clip_launch(name, nch, fmt, n, size, k):
    """Packets of 1 frame, 7, 97, exactly orig, one shorter than the largest carry, and enough to emit more than half the ring; the
    ring (600 samples) starts just before its end, so the first tile wraps, and wraps again every other packet."""
    sizes = split(n, int(size))
    run_chain(name, nch, fmt, n, sizes, RING, seed=777 + k, ring_start=RING - 3, misalign=0)


@pytest.mark.parametrize("fmt", ["s16", "f32"])
def test_a_packet_one_sample_off_16_byte_alignment(fmt):
    run_chain("441:160", 2, fmt, 1500, [441, 7, 500, 552], RING, seed=31, ring_start=5, misalign=2 if fmt == "s16" else 4)


def test_half_ring_packets_with_mixed_empty_and_tiny_ones():
    """0-frame packets, packets too short for a group (the carry alone moves), and the largest that still fits, on 8 channels."""
    _, orig, nw, width = GEOM["3:1"]
    run_chain("3:1", 8, "s16", 2 * 1797 + 4 + 35, [0, 1, 1797, 0, 2, 35, 1797, 1], RING, seed=5, ring_start=RING - 1)


def test_three_streams_of_three_rates_in_one_launch():
    specs = [("3:1", 2, "s16", 1920), ("441:160", 1, "f32", 1764), ("1:1", 3, "s16", 640)]
    per = [96 * 2, 441 // 3 + 30, 64]      # what each sender's packet holds: 10 launches carry every signal
    lanes, sigs = [], []
    for i, (name, nch, fmt, n) in enumerate(specs):
        pcm, x = pcm_signal(fmt, nch, n, 90 + i)
        lanes.append(Lane(name, nch, fmt, 257, max(per), ring_start=250 + i))
        sigs.append((pcm, x))
    at = [0, 0, 0]
    while any(at[i] < specs[i][3] for i in range(3)):
        pkts = []
        for i in range(3):
            n = specs[i][3]
            s = min(per[i], n - at[i])
            pkts.append(sigs[i][0][at[i]:at[i] + s])
            at[i] += s
        launch(lanes, pkts)
    assert at == [s[3] for s in specs]
    launch(lanes, [None] * 3, end=True)
    for ln, (name, nch, fmt, n), (pcm, x) in zip(lanes, specs, sigs):
        got, want = torch.cat(ln.outs), whole_clip(name, x)
        assert got.shape == want.shape and torch.equal(bits(got), bits(want)), name


def test_s16_is_the_float_of_the_same_integers():
    """An s16 stream and an f32 stream fed value / 32768 of the same integers give the same bits."""
    pcm, _ = pcm_signal("s16", 2, 1000, 11)
    pcm[0, 0], pcm[1, 1], pcm[2, 0] = -32768, 32767, 0
    x = (pcm.astype(np.float32) / np.float32(32768.0)).T
    a, b = Lane("3:1", 2, "s16", RING, 1000), Lane("3:1", 2, "f32", RING, 1000)
    launch([a, b], [pcm, np.ascontiguousarray(x.T)])
    launch([a, b], [None, None], end=True)
    assert torch.equal(bits(torch.cat(a.outs)), bits(torch.cat(b.outs)))


# ---------------------------------------------------------------------------------------------- take
def test_take_gathers_across_the_wrap_and_zero_fills():
    L = capi.lib()
    block, cap, stride = 640, 1500, 700
    g = torch.Generator().manual_seed(3)
    rings = [torch.randn(cap, generator=g).cuda() for _ in range(3)]
    spec = [(1400, 640), (0, 640), (1499, 37)]                          # (read position, n_valid): across the wrap; plain; a short last row
    descs = (capi.PcmTakeDesc * 3)(*[capi.PcmTakeDesc(ring=r.data_ptr(), ring_cap=cap, read_pos=p, n_valid=v) for r, (p, v) in zip(rings, spec)])
    table = torch.zeros(3 * C.sizeof(capi.PcmTakeDesc), dtype=torch.uint8, device="cuda")
    buf = torch.full((GUARD + 4 * stride + GUARD,), float("nan"), dtype=torch.float32, device="cuda")
    rings0 = [bits(r).clone() for r in rings]
    for n in (3, 2):                                                    # all three rows; then two: the third row stays as it is
        buf.fill_(float("nan"))
        rc = L.artalk_op_pcm_take(descs, n, capi.ptr(table), table.numel(), capi.ptr(buf[GUARD:]), stride, block, capi.current_stream_ptr())
        torch.cuda.synchronize()
        assert rc == capi.OK
        rows = buf[GUARD:GUARD + 4 * stride].view(4, stride)
        for i, (r, (p, v)) in enumerate(zip(rings, spec)):
            if i >= n:
                assert torch.isnan(rows[i]).all(), "a row of a stream that was not listed was written"
                continue
            want = torch.zeros(block, device="cuda")
            want[:v] = r[(p + torch.arange(v, device="cuda")) % cap]
            assert torch.equal(bits(rows[i, :block]), bits(want)), f"row {i}"
            assert torch.isnan(rows[i, block:]).all(), "the gap between two rows was written"
        assert torch.isnan(rows[3]).all() and torch.isnan(buf[:GUARD]).all() and torch.isnan(buf[GUARD + 4 * stride:]).all()
        assert all(torch.equal(bits(r), r0) for r, r0 in zip(rings, rings0)), "a ring was written"
