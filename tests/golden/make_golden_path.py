"""Generate tests/golden/ref_path.npz by IMPORTING the reference's own utils/render_utils.py and running its path generator on two
seeded camera sets.  Runs only in the build container (needs /root/reference); the .npz (arrays only) is committed.

Stand-ins: `mediapy` (not installed; only create_videos uses it) is an empty module in sys.modules; torch.Tensor.cuda is the identity
for the call (no GPU in the build container).

Camera sets (world_view_transform fp32, as a Camera stores it):
  ring   12 cameras on a jittered ring around the origin, looking inwards: an object-centric 360-degree capture
  dome    9 cameras on one side of a dome, looking at a point below it: a DTU-like capture
Both are checked to have distinct PCA eigenvalues (the eigenvectors' order, hence the whole path, depends on them).

Recorded per set: the inputs (wvt [N,4,4] fp32, height, width — odd on purpose); transform_poses_pca's (poses_recentered, transform) on
the OpenGL-convention poses; generate_ellipse_path(poses_recentered, n) and generate_path(cameras, n)'s world_view_transform (fp32) for
n in {8, 240}.

Usage:  python tests/golden/make_golden_path.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "tests"))

import path_scenes as PS  # noqa: E402


def main():
    sys.modules.setdefault("mediapy", types.ModuleType("mediapy"))
    sys.path.insert(0, REF)
    from utils import render_utils as RU
    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    out = {}
    try:
        for name in PS.SETS:
            wvt, H, W = PS.camera_set(name)
            cams = [types.SimpleNamespace(world_view_transform=torch.from_numpy(w), projection_matrix=torch.from_numpy(PS.projection(H, W)),
                                          image_height=H, image_width=W) for w in wvt]
            c2ws = np.array([np.linalg.inv(np.asarray(c.world_view_transform.T.numpy())) for c in cams])
            pose = c2ws[:, :3, :] @ np.diag([1, -1, -1, 1])
            t = pose[:, :3, 3] - pose[:, :3, 3].mean(0)
            ev = np.sort(np.linalg.eigvalsh(t.T @ t))
            assert np.all(np.diff(ev) > 1e-3 * ev[-1]), (name, ev)
            rec, tr = RU.transform_poses_pca(pose)
            out[name + "/wvt"], out[name + "/size"] = wvt, np.array([H, W])
            out[name + "/pose"], out[name + "/recentered"], out[name + "/transform"] = pose, rec, tr
            out[name + "/focus"] = RU.focus_point_fn(rec)
            for n in (8, 240):
                out["%s/ellipse%d" % (name, n)] = RU.generate_ellipse_path(rec, n_frames=n)
                traj = RU.generate_path(cams, n_frames=n)
                assert all((c.image_height, c.image_width) == (H // 2 * 2, W // 2 * 2) for c in traj)
                out["%s/path%d" % (name, n)] = np.stack([c.world_view_transform.numpy() for c in traj])
                assert out["%s/path%d" % (name, n)].dtype == np.float32
    finally:
        torch.Tensor.cuda = cuda
    path = os.path.join(HERE, "ref_path.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d arrays, %d bytes)" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
