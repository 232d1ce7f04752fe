"""Portable f16x3 site scales without a GPU: the save_scales / load_scales file and its validation (the library calls stubbed out),
and the rank agreement of artalk_amd.dist.agree_scales_dict on the gloo backend at world size 2 and 8."""
import json
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from artalk_amd.config import ARTalkConfig
from artalk_amd.dist import agree_scales_dict
from artalk_amd.model import SCALES_FORMAT, BitwiseARModel, check_scales, read_scales_file

NAMES = ["w2v.conv0.ln_gelu", "w2v.feature_projection.ln", "w2v.layer0.ffn_hidden", "ar.block0.ln1_mod", "style.input(fp32 A)"]


class _StubLib:
    """The model's three library hooks replaced by a host list: what artalk_set_site_scales would hold."""
    def __init__(self, model, names):
        self.exps = [4] * len(names)
        self.writes = 0
        model._loaded = True
        model._site_names = lambda: list(names)
        model._read_site_exps = lambda: list(self.exps)
        model._write_site_exps = self._write

    def _write(self, exps):
        self.writes += 1
        changed = sum(a != b for a, b in zip(self.exps, exps))
        self.exps = list(exps)
        return changed


def _model():
    m = BitwiseARModel(ARTalkConfig.tiny())
    return m, _StubLib(m, NAMES)


def test_save_load_round_trip(tmp_path):
    a, la = _model()
    la.exps = [4, -2, 1, 4, 3]
    a._headroom = 4.0
    path = str(tmp_path / "scales.json")
    a.save_scales(path)
    doc = json.load(open(path))
    assert doc["format"] == SCALES_FORMAT and doc["headroom"] == 4.0
    assert list(doc["sites"]) == NAMES and list(doc["sites"].values()) == [4, -2, 1, 4, 3]
    assert doc["config"]["ar_depth"] == ARTalkConfig.tiny().ar_depth
    assert read_scales_file(path)["sites"] == a.scales()
    b, lb = _model()
    assert b.load_scales(path) == 3
    assert b.scales() == a.scales() and b._headroom == 4.0
    assert b.load_scales(path) == 0                        # the same values again: nothing changes
    assert b.load_scales({n: 4 for n in NAMES}) == 3 and lb.exps == [4] * 5      # a dict works as well


def _bad_cases():
    good = {n: 4 for n in NAMES}
    missing = dict(good)
    missing.pop("ar.block0.ln1_mod")
    extra = dict(good, **{"ar.block99.ffn_hidden": 4})
    return [
        ("missing", missing, "missing"),
        ("extra", extra, "extra"),
        ("exp5", dict(good, **{NAMES[1]: 5}), r"outside \[-8, 4\]"),
        ("exp-9", dict(good, **{NAMES[1]: -9}), r"outside \[-8, 4\]"),
        ("float", dict(good, **{NAMES[2]: 2.0}), "not an int"),
        ("str", dict(good, **{NAMES[2]: "2"}), "not an int"),
        ("bool", dict(good, **{NAMES[2]: True}), "not an int"),
    ]


@pytest.mark.parametrize("kind,sites,match", _bad_cases(), ids=[c[0] for c in _bad_cases()])
def test_load_rejects_before_the_library_is_called(tmp_path, kind, sites, match):
    m, lib = _model()
    with pytest.raises(ValueError, match=match):
        m.load_scales(sites)
    path = str(tmp_path / "s.json")
    json.dump({"format": SCALES_FORMAT, "sites": sites, "config": {}, "headroom": None}, open(path, "w"))
    with pytest.raises(ValueError, match=match):
        m.load_scales(path)
    assert lib.writes == 0 and lib.exps == [4] * len(NAMES)


def test_missing_and_extra_names_are_listed():
    sites = {n: 4 for n in NAMES[1:]}
    sites["vae.decoder.layer9.qkv"] = 4
    with pytest.raises(ValueError) as e:
        check_scales(sites, NAMES)
    assert "w2v.conv0.ln_gelu" in str(e.value) and "vae.decoder.layer9.qkv" in str(e.value)


def test_wrong_format_tag_is_rejected(tmp_path):
    m, lib = _model()
    path = str(tmp_path / "s.json")
    for fmt in ("artalk-site-scales/2", None):
        json.dump({"format": fmt, "sites": {n: 4 for n in NAMES}}, open(path, "w"))
        with pytest.raises(ValueError, match="format"):
            m.load_scales(path)
    json.dump([1, 2], open(path, "w"))
    with pytest.raises(ValueError, match="format"):
        m.load_scales(path)
    assert lib.writes == 0


# ---------------------------------------------------------------------------------------------- dict-level MIN agreement on gloo
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_sites(rank, world):
    """Rank r starts from its own exponents: a deterministic pattern in [-8, 4] that differs per rank and per site."""
    return {n: 4 - ((rank * 5 + 3 * i) % 13) for i, n in enumerate(NAMES)}


def _worker(rank, world, port, mismatch, q):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(1)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        sites = _rank_sites(rank, world)
        if mismatch and rank == world - 1:
            sites = dict(sites)
            sites.pop(NAMES[-1])
            sites["style.layer7.ffn_hidden(fp32 A)"] = 4
        try:
            got = agree_scales_dict(sites)
            want = {n: min(_rank_sites(r, world)[n] for r in range(world)) for n in NAMES}
            ok = (not mismatch) and got == want and list(got) == list(sites)
        except RuntimeError as e:
            ok = mismatch and "site lists differ" in str(e)
    except Exception as e:      # noqa: BLE001 - reported through the queue
        ok = False
        print(f"rank {rank}: {type(e).__name__}: {e}", flush=True)
    q.put((rank, ok))
    dist.destroy_process_group()


def _run(world, mismatch):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, mismatch, q)) for r in range(world)]
    for p in procs:
        p.start()
    results = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(results) == [(r, True) for r in range(world)]


@pytest.mark.parametrize("world", [2, 8])
def test_agree_scales_takes_the_elementwise_minimum(world):
    _run(world, mismatch=False)


@pytest.mark.parametrize("world", [2, 8])
def test_agree_scales_raises_on_every_rank_when_site_lists_differ(world):
    _run(world, mismatch=True)
