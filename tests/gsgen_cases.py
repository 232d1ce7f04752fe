"""Case table of the Gaussian generators' tests (tests/test_gsgen_cpu.py, test_gsgen_ops_gpu.py, test_gsgen_gpu.py) and of
tools/make_golden_gsgen.py: the smallest shapes at which the paths still differ.  Weights come from
artalk_amd.gsgen.synth_state_dict(*dims, seed=SEED) and are not stored; features and transforms are rebuilt here from seeds."""
import math

import numpy as np

SEED = 0
# (V, Dh, Dg, C, P)
CASES = {
    "A": (50, 16, 48, 16, 6),          # 36 pixels, less than one 128-pixel tile; Cin = 43 takes the element-wise loads; hidden 8
    "B": (130, 24, 40, 24, 12),        # 144 pixels and 130 rows each cross a tile boundary; hidden 12 is not a multiple of 8
    "C": (33, 256, 768, 256, 5),       # the reference's channel widths: K = 2547 and 1152 through all three sum levels, Cout 128 and 41
    "D": (128, 16, 16, 32, 16),        # 256 pixels and 128 rows: exact tiles
}
REFERENCE_DIMS = (5023, 256, 768, 256, 296)
ATTRS = {"xyz": 3, "colors": 32, "opacities": 1, "scales": 3, "rotations": 4}
# per case: rotation axis (skew), angle, translation
_POSES = {
    "A": ((0.3, -0.8, 0.5), 0.41, (0.031, -0.114, 9.61)),
    "B": ((-0.6, 0.2, 0.75), -0.27, (-0.08, 0.05, 9.9)),
    "C": ((0.5, 0.5, -0.7), 0.63, (0.12, 0.02, 9.2)),
    "D": ((-0.2, -0.9, -0.4), 1.1, (0.0, -0.21, 10.4)),
}


def transform_matrix(name):
    """(3, 4) float32 [R | t]: a rotation about a skew axis beside diag(-1, 1, -1) (the frontal camera of the head's tests) and a
    translation."""
    axis, angle, t = _POSES[name]
    a = np.asarray(axis, dtype=np.float64)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    R = (np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * K @ K) @ np.diag([-1.0, 1.0, -1.0])
    return np.concatenate([R, np.asarray(t, dtype=np.float64)[:, None]], axis=1).astype(np.float32)


def features(name):
    """f_feature0 (C, P, P) and f_feature1 (Dg,), float32, standard normal."""
    V, Dh, Dg, C, P = CASES[name]
    g = np.random.Generator(np.random.SFC64(4000 + ord(name)))
    return g.standard_normal((C, P, P), dtype=np.float32), g.standard_normal(Dg, dtype=np.float32)


def n_gaussians(name):
    V, _, _, _, P = CASES[name]
    return V + 2 * P * P


FACTOR = 4.0      # the project's rule for a float32 kernel: max-abs error <= 4 x e32, with a floor of one float32 ulp of the largest value
_runs = {}


def allowance(e32, largest):
    return max(FACTOR * e32, float(np.spacing(np.float32(largest))))


def reference_run(name):
    """Per case, computed once and read only: the weights, the inputs, the restatement in float64 and, per attribute, e32 (the
    restatement in float32 against float64 on the CPU: what a float32 evaluation loses by itself) and the allowance made of it."""
    if name not in _runs:
        import torch
        from artalk_amd.gsgen import synth_state_dict
        from gsgen_ref import generate
        sd = synth_state_dict(*CASES[name], seed=SEED)
        f0, f1 = features(name)
        tm = transform_matrix(name)
        with torch.no_grad():
            want = generate(sd, f0, f1, tm, torch.float64)
            got32 = generate(sd, f0, f1, tm, torch.float32)
        e32 = {k: float((got32[k].double() - want[k]).abs().max()) for k in ATTRS}
        allow = {k: allowance(e32[k], float(want[k].abs().max())) for k in ATTRS}
        _runs[name] = dict(sd=sd, f0=f0, f1=f1, tm=tm, want=want, e32=e32, allow=allow)
    return _runs[name]
