"""Generate tests/golden/ref_eval.npz by running the reference's own scripts/eval_dtu/eval.py on the synthetic DTU-shaped scene of
tests/eval_scenes.py (EVAL.md §Pinning).

eval.py needs Open3D only to read two files and to write two; a stand-in `open3d` module routes those through surfel_io.  Its shuffle
is unseeded, so numpy.random.default_rng is wrapped to hand the unseeded call a chosen seed.  Everything else (numpy, scikit-learn's
KD-tree, scipy.io.loadmat, the multiprocessing pool) is the reference's own code path.  The fixture holds data only: the generator's
parameters, the reference's three means and its stage sizes per parameter set and seed.

Runs only where the reference checkout (REF_ROOT, default ../../../reference relative to this file), scikit-learn and scipy exist.
    python tests/golden/make_golden_eval.py            writes ref_eval.npz
    python tests/golden/make_golden_eval.py --time     times one run on eval_scenes.SCALED (prints, writes nothing)
"""
import json
import os
import runpy
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF_ROOT", os.path.join(REPO, "..", "reference"))
sys.path.insert(0, os.path.join(REPO, "2d-gaussian-splatting_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import eval_scenes as S  # noqa: E402
import surfel_io  # noqa: E402


class _Geom:
    pass


def _stand_in_open3d():
    o3d = types.ModuleType("open3d")

    def read_triangle_mesh(path):
        v, t, _ = surfel_io.read_triangle_mesh(path)
        m = _Geom()
        m.vertices, m.triangles = v.astype(np.float64), t
        return m

    def read_point_cloud(path):
        p = surfel_io.read_ply(path)
        c = _Geom()
        c.points = np.stack([p["x"], p["y"], p["z"]], 1).astype(np.float64)
        return c

    def write_point_cloud(path, pcd):
        m = _Geom()
        m.vertices, m.vertex_colors, m.triangles = np.asarray(pcd.points), np.asarray(pcd.colors), np.zeros((0, 3), np.int32)
        surfel_io.write_triangle_mesh(path, m)

    o3d.io = types.SimpleNamespace(read_triangle_mesh=read_triangle_mesh, read_point_cloud=read_point_cloud, write_point_cloud=write_point_cloud)
    o3d.geometry = types.SimpleNamespace(PointCloud=_Geom)
    o3d.utility = types.SimpleNamespace(Vector3dVector=np.asarray)
    return o3d


def write_dataset(root, scene=S.FIXTURE, scan=1):
    from scipy.io import savemat
    os.makedirs(os.path.join(root, "ObsMask"))
    os.makedirs(os.path.join(root, "Points", "stl"))
    mask, bb, res, plane = S.fixture_obs(scene)
    savemat(os.path.join(root, "ObsMask", "ObsMask%d_10.mat" % scan), {"ObsMask": mask, "BB": bb, "Res": res})
    savemat(os.path.join(root, "ObsMask", "Plane%d.mat" % scan), {"P": plane.reshape(4, 1)})
    surfel_io.write_ply(os.path.join(root, "Points", "stl", "stl%03d_total.ply" % scan), ["x", "y", "z"], S.fixture_ground_truth(scene))
    v, t = S.fixture_mesh(scene)
    m = _Geom()
    m.vertices, m.triangles, m.vertex_colors = v, t, np.zeros_like(v)
    surfel_io.write_triangle_mesh(os.path.join(root, "mesh.ply"), m)


def run_reference(root, out, params, seed, scan=1):
    """The namespace of eval.py run as __main__ on the dataset under root, its unseeded shuffle seeded with `seed`."""
    rng = np.random.default_rng
    argv = sys.argv
    sys.modules["open3d"] = _stand_in_open3d()
    np.random.default_rng = lambda s=None: rng(seed if s is None else s)
    sys.argv = ["eval.py", "--data", os.path.join(root, "mesh.ply"), "--scan", str(scan), "--mode", "mesh", "--dataset_dir", root, "--vis_out_dir", out,
                "--downsample_density", repr(params["density"]), "--patch_size", repr(params["patch"]), "--max_dist", repr(params["max_dist"])]
    try:
        return runpy.run_path(os.path.join(REF, "scripts", "eval_dtu", "eval.py"), run_name="__main__")
    finally:
        np.random.default_rng, sys.argv = rng, argv
        del sys.modules["open3d"]


SIZES = ("data_pcd", "data_down", "data_in", "data_in_obs", "stl_above")


def main():
    with tempfile.TemporaryDirectory() as root:
        if "--time" in sys.argv:
            write_dataset(root, S.SCALED)
            t0 = time.perf_counter()
            ns = run_reference(root, root, S.PARAMS[0], 0)
            print("reference eval.py: %d samples, %d kept, %d ground-truth points, overall %.6f, %.1f s on %d CPUs"
                  % (len(ns["data_pcd"]), len(ns["data_down"]), len(ns["stl"]), ns["over_all"], time.perf_counter() - t0, os.cpu_count()))
            return
        write_dataset(root)
        means = np.zeros((len(S.PARAMS), len(S.SEEDS), 3))
        sizes = np.zeros((len(S.PARAMS), len(S.SEEDS), len(SIZES)), np.int64)
        for a, params in enumerate(S.PARAMS):
            for b, seed in enumerate(S.SEEDS):
                ns = run_reference(root, root, params, seed)
                means[a, b] = ns["mean_d2s"], ns["mean_s2d"], ns["over_all"]
                sizes[a, b] = [len(ns[k]) for k in SIZES]
                res = json.load(open(os.path.join(root, "results.json")))
                assert res["mean_d2s"] == means[a, b, 0] and res["overall"] == means[a, b, 2]
                print(params, seed, means[a, b], sizes[a, b])
    np.savez(os.path.join(HERE, "ref_eval.npz"), scene=json.dumps(S.FIXTURE), params=json.dumps(S.PARAMS), seeds=np.array(S.SEEDS), means=means,
             sizes=sizes, size_names=np.array(SIZES))


if __name__ == "__main__":
    main()
