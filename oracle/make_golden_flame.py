#!/usr/bin/env python
"""tests/golden/flame_lbs.npz and tests/golden/flame_lbs_joints.npz from the REFERENCE's own lbs() (build container only): imports
/root/reference/app/flame_model/lbs.py by path (its package __init__ pulls pytorch3d, which is absent) and runs it on the
deterministic synthetic FLAME asset with inputs shaped like the engine's (inference.py:62-69: zero shape code, codes (T,106)).
  flame_lbs.npz         T = 6, global and jaw pose, neck and eyes at rest (what FLAMEModel.forward gets from the engine)
  flame_lbs_joints.npz  T = 4, all 15 pose components non-zero, shape and expression = the first four rows of the former
A fixture whose arrays come out bit for bit as the committed file holds them is left alone (a zip archive carries time stamps)."""
import importlib.util
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from artalk_amd.flame import synthetic_flame_asset  # noqa: E402

spec = importlib.util.spec_from_file_location("ref_lbs", "/root/reference/app/flame_model/lbs.py")
ref = importlib.util.module_from_spec(spec)
sys.dont_write_bytecode = True
spec.loader.exec_module(ref)

asset = synthetic_flame_asset()
fm = asset["flame_model"]
sd = fm["shapedirs"]
shapedirs = torch.cat([sd[:, :, :300], sd[:, :, 300:400]], 2)
posedirs = fm["posedirs"].reshape(-1, 36).T
parents = fm["kintree_table"][0].clone(); parents[0] = -1


def ref_lbs(betas, full_pose):
    T = betas.shape[0]
    verts, _ = ref.lbs(betas, full_pose, fm["v_template"][None].expand(T, -1, -1), shapedirs, posedirs, fm["J_regressor"], parents,
                       fm["weights"], dtype=torch.float32, detach_pose_correctives=False)
    return verts


def write(name, verts, **inputs):
    out = os.path.join(REPO, "tests", "golden", name)
    arrays = dict(inputs, verts_sub=verts[:, ::37].numpy().astype(np.float32), verts_sum=np.float64(verts.double().sum().item()),
                  verts_abs_mean=np.float64(verts.abs().double().mean().item()))
    if os.path.exists(out):
        with np.load(out) as old:
            if sorted(old.files) == sorted(arrays) and all(old[k].dtype == np.asarray(v).dtype and old[k].tobytes() == np.asarray(v).tobytes()
                                                           for k, v in arrays.items()):
                print("unchanged", out, tuple(verts.shape))
                return
    np.savez_compressed(out, **arrays)
    print("wrote", out, os.path.getsize(out) // 1024, "KiB", tuple(verts.shape), float(verts.abs().max()))


g = torch.Generator().manual_seed(3)
T = 6
shape = 0.5 * torch.randn(T, 300, generator=g)
shape[0] = 0.0                                      # the engine's default shape code (inference.py:63)
motion = torch.cat([torch.randn(T, 100, generator=g), 0.3 * torch.randn(T, 6, generator=g)], dim=1)   # (T,106)
exp, pose = motion[:, :100], motion[:, 100:]
betas = torch.cat([shape, exp], dim=1)
full_pose = torch.cat([pose[:, :3], torch.zeros(T, 3), pose[:, 3:], torch.zeros(T, 6)], dim=1)
write("flame_lbs.npz", ref_lbs(betas, full_pose), shape=shape.numpy(), motion=motion.numpy())

# all five joints: global, neck, jaw, left eye, right eye in the order of lbs()'s pose argument (FLAME.py:137-141)
TJ = 4
full_pose5 = 0.3 * torch.randn(TJ, 15, generator=torch.Generator().manual_seed(5))
assert (full_pose5 != 0).all()
write("flame_lbs_joints.npz", ref_lbs(betas[:TJ].contiguous(), full_pose5), shape=shape[:TJ].numpy(), exp=exp[:TJ].contiguous().numpy(),
      full_pose=full_pose5.numpy())
