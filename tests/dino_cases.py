"""Case table of the DINO-feature tests (tests/test_dino_cpu.py, test_dino_ops_gpu.py, test_dino_gpu.py) and of
tools/make_golden_dino.py: the smallest shapes at which the paths still differ.  Weights come from
artalk_amd.dino.synth_state_dict(*dims, seed=SEED) and are not stored; images are rebuilt here from seeds.  The head's hidden width 256
and its projection widths 256 / 512 / 1024 / 1024 are the reference's constants at every case."""
import numpy as np

SEED = 0
# (output_dim, vit_dim, depth, heads, grid)
CASES = {
    "A": (16, 128, 5, 2, 5),      # 26 tokens; odd sizes 5 -> 20 / 10 / 5 / 3 -> 40; depth 5 tells "the last four" from "all"; heads of 64
    "B": (16, 64, 4, 2, 6),       # 37 tokens; even sizes 6 -> 3; heads of 32: the 32-wide attention kernel; a LayerNorm width of 64
    "C": (8, 128, 4, 2, 9),       # 82 tokens: two 64-key blocks, the second partial; a partial 128-pixel conv tile at 5 x 5 and 9 x 9
}
REFERENCE_DIMS = (256, 768, 12, 12, 37)
OUTPUTS = ("plane", "glob")


def image(name):
    """(3, 14 g, 14 g) float32 in [0, 1): white noise on a ramp, so that antialiasing and the resize geometry both matter."""
    g = CASES[name][4]
    S = 14 * g
    r = np.random.Generator(np.random.SFC64(5000 + ord(name)))
    ramp = np.linspace(0.0, 0.5, S, dtype=np.float32)
    return (0.5 * r.random((3, S, S), dtype=np.float32) + ramp[None, :, None] * ramp[None, None, :] * 2).astype(np.float32)


FACTOR = 4.0      # the project's rule for a float32 kernel: max-abs error <= 4 x e32, with a floor of one float32 ulp of the largest value
_runs = {}


def allowance(e32, largest):
    return max(FACTOR * e32, float(np.spacing(np.float32(largest))))


def _flat(run):
    out = {"plane": run["plane"], "glob": run["glob"]}
    for i in range(4):
        out[f"tap{i}"] = run["taps"][i]
        out[f"rn{i}"] = run["rn"][i]
    return out


def reference_run(name):
    """Per case, computed once and read only: the weights, the image, the restatement in float64 and, per output and intermediate, e32
    (the restatement in float32 against float64 on the CPU: what a float32 evaluation loses by itself) and the allowance made of it."""
    if name not in _runs:
        import torch
        from artalk_amd.dino import synth_state_dict
        from dino_ref import forward
        dims = CASES[name]
        sd = synth_state_dict(*dims, seed=SEED)
        img = image(name)
        with torch.no_grad():
            want = _flat(forward(sd, img, dims, torch.float64))
            got32 = _flat(forward(sd, img, dims, torch.float32))
        e32 = {k: float((got32[k].double() - want[k]).abs().max()) for k in want}
        allow = {k: allowance(e32[k], float(want[k].abs().max())) for k in want}
        _runs[name] = dict(sd=sd, image=img, want=want, e32=e32, allow=allow, dims=dims)
    return _runs[name]
