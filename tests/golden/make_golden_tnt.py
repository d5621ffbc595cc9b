"""Generate tests/golden/ref_tnt.npz by running the reference's own scripts/eval_tnt/run.py::run_evaluation on the synthetic
Tanks-and-Temples-shaped directory of tests/tnt_scenes.py (TNT.md §Pinning).

run.py, registration.py, evaluation.py, trajectory_io.py, config.py and plot.py are the reference's own code; Open3D and trimesh, which
they import, do not exist here.  Stand-in `open3d` and `trimesh` modules map the primitives they call onto tests/tnt_oracle.py and
surfel_io, with Open3D's signatures — in particular ICPConvergenceCriteria(relative_fitness, relative_rmse, max_iteration = 30), which the
reference fills positionally.  matplotlib is real (Agg).  The fixture therefore pins what the reference's Python decides: the stage
order, the thresholds 80 / 20 / 2 tau, the voxel sizes, T_icp . T_init, the centroid augmentation, get_f1_score_histo2 and its edges.
Open3D's primitives themselves are pinned only to the oracle.  The fixture holds data only: the generator's parameters and the recorded
results per case.

The second case (relative_rmse = 1e-6) cannot be reached through run.py's hard-coded call; for it the stand-in's ICPConvergenceCriteria
overrides the arguments it is given with the case's.

Runs only where the reference checkout (REF_ROOT, default ../../../reference relative to this file), scipy and matplotlib exist.
    python tests/golden/make_golden_tnt.py            writes ref_tnt.npz
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.environ.get("REF_ROOT", os.path.join(REPO, "..", "reference"))
sys.path.insert(0, os.path.join(REPO, "2d-gaussian-splatting_amd"))
sys.path.insert(0, os.path.join(REPO, "tests"))
import tnt_oracle as O  # noqa: E402
import tnt_scenes as S  # noqa: E402
import surfel_io  # noqa: E402

LOG = {"stages": [], "crops": [], "transforms": [], "scored": [], "criteria": None, "trajectory": None}


class PointCloud:
    def __init__(self, points=None):
        self.points = [] if points is None else np.asarray(points, np.float64).reshape(-1, 3)
        self.colors = None

    def arr(self):
        return np.asarray(self.points, np.float64).reshape(-1, 3)

    def transform(self, T):
        LOG["transforms"].append(np.array(T, np.float64))
        self.points = O.transform(self.arr(), T)
        return self

    def voxel_down_sample(self, voxel_size):
        return PointCloud(O.voxel_down_sample(self.arr(), voxel_size)[0])

    def uniform_down_sample(self, every_k_points):
        return PointCloud(self.arr()[::every_k_points])

    def estimate_normals(self, search_param=None):
        pass

    def compute_point_cloud_distance(self, target):
        LOG["scored"].append(len(self.arr()))
        return O.nearest(self.arr(), target.arr())[0]


class _Volume:
    def __init__(self, path):
        with open(path) as f:
            d = json.load(f)
        self.vol = O.CropVolume(d["orthogonal_axis"], d["axis_min"], d["axis_max"], d["bounding_polygon"])

    def crop_point_cloud(self, pcd):
        out = PointCloud(O.crop(pcd.arr(), self.vol))
        LOG["crops"].append((len(pcd.arr()), len(out.arr())))
        return out


def _stand_in_open3d(case, ransac_seed):
    o3d = types.ModuleType("open3d")

    def read_point_cloud(path):
        p = surfel_io.read_ply(path)
        return PointCloud(np.stack([p["x"], p["y"], p["z"]], 1))

    def write_point_cloud(path, pcd):
        m = types.SimpleNamespace(vertices=pcd.arr(), vertex_colors=np.asarray(pcd.colors), triangles=np.zeros((0, 3), np.int32))
        surfel_io.write_triangle_mesh(path, m)

    def icp_criteria(relative_fitness=1e-6, relative_rmse=1e-6, max_iteration=30):      # Open3D's signature and defaults
        given = dict(relative_fitness=relative_fitness, relative_rmse=relative_rmse, max_iteration=max_iteration)
        if LOG["criteria"] is None:
            LOG["criteria"] = given
        return types.SimpleNamespace(**(case or given))

    def registration_icp(source, target, max_correspondence_distance, init, estimation, criteria):
        assert estimation.with_scaling
        r = O.icp_similarity(source.arr(), target.arr(), max_correspondence_distance, init, criteria.relative_fitness, criteria.relative_rmse,
                             criteria.max_iteration)
        LOG["stages"].append({"threshold": max_correspondence_distance, "source": len(source.arr()), "target": len(target.arr()),
                              "iterations": r["iterations"], "fitness": r["fitness"], "inlier_rmse": r["inlier_rmse"]})
        return types.SimpleNamespace(transformation=r["transformation"], fitness=r["fitness"], inlier_rmse=r["inlier_rmse"])

    def registration_ransac(source, target, corres, max_correspondence_distance, estimation, ransac_n, criteria):
        corres = np.asarray(corres)
        assert estimation.with_scaling and np.array_equal(corres[:, 0], corres[:, 1]) and np.array_equal(corres[:, 0], np.arange(len(source.arr())))
        T, fit, rmse = O.trajectory_alignment(source.arr(), target.arr(), None, ransac_seed, max_correspondence_distance, ransac_n, criteria.max_iteration)
        LOG["trajectory"] = {"transformation": T, "fitness": fit, "inlier_rmse": rmse}
        return types.SimpleNamespace(transformation=T, fitness=fit, inlier_rmse=rmse)

    o3d.io = types.SimpleNamespace(read_point_cloud=read_point_cloud, write_point_cloud=write_point_cloud)
    o3d.geometry = types.SimpleNamespace(PointCloud=PointCloud, KDTreeSearchParamKNN=lambda knn=30: None)
    o3d.utility = types.SimpleNamespace(Vector3dVector=lambda a: np.asarray(a, np.float64), Vector2iVector=lambda a: np.asarray(a, np.int64),
                                        set_verbosity_level=lambda level: None, VerbosityLevel=types.SimpleNamespace(Debug=0))
    o3d.visualization = types.SimpleNamespace(read_selection_polygon_volume=_Volume, draw_geometries=lambda g: None)
    o3d.registration = types.SimpleNamespace(
        RANSACConvergenceCriteria=lambda: types.SimpleNamespace(max_iteration=1000, max_validation=1000),
        TransformationEstimationPointToPoint=lambda with_scaling=False: types.SimpleNamespace(with_scaling=with_scaling),
        ICPConvergenceCriteria=icp_criteria, registration_icp=registration_icp,
        registration_ransac_based_on_correspondence=registration_ransac)
    return o3d


def _stand_in_trimesh():
    tm = types.ModuleType("trimesh")

    def load_mesh(path):
        v, t, _ = surfel_io.read_triangle_mesh(path)
        return types.SimpleNamespace(vertices=v.astype(np.float64), faces=t)

    tm.load_mesh = load_mesh
    return tm


def write_trajectory_log(path, poses):
    with open(path, "w") as f:
        for i, p in enumerate(poses):
            f.write("%d %d 0\n" % (i, i))
            f.write("\n".join(" ".join("{0:.12f}".format(x) for x in row) for row in p.tolist()) + "\n")


def write_dataset(root, scene=S.FIXTURE):
    """root/SCENE with the four files run.py:74-81 expects, the mesh and the estimated trajectory beside it."""
    name = scene["scene"]
    d = os.path.join(root, name)
    os.makedirs(d)
    surfel_io.write_ply(os.path.join(d, name + ".ply"), ["x", "y", "z"], S.ground_truth(scene))
    with open(os.path.join(d, name + ".json"), "w") as f:
        json.dump(dict(S.crop_fields(scene), class_name="SelectionPolygonVolume", version_major=1, version_minor=0), f)
    est, col = S.cameras(scene)
    write_trajectory_log(os.path.join(d, name + "_COLMAP_SfM.log"), col)
    np.savetxt(os.path.join(d, name + "_trans.txt"), S.alignment(scene))
    np.save(os.path.join(root, "traj.npy"), est)
    v, t = S.mesh(scene)
    surfel_io.write_triangle_mesh(os.path.join(root, "mesh.ply"), types.SimpleNamespace(vertices=v, triangles=t, vertex_colors=np.zeros_like(v)))
    return d


def run_reference(root, dataset_dir, case):
    """run.py::run_evaluation on the dataset; case None: the criteria the reference itself passes."""
    import matplotlib
    matplotlib.use("Agg")
    for k in LOG:
        LOG[k] = [] if isinstance(LOG[k], list) else None
    mods = ("open3d", "trimesh", "run", "registration", "evaluation", "trajectory_io", "config", "plot", "util")
    for m in mods:
        sys.modules.pop(m, None)
    sys.modules["open3d"], sys.modules["trimesh"] = _stand_in_open3d(case, S.RANSAC_SEED), _stand_in_trimesh()
    sys.path.insert(0, os.path.join(REF, "scripts", "eval_tnt"))
    out = os.path.join(root, "evaluation")
    try:
        import run
        with contextlib.redirect_stdout(io.StringIO()):
            run.run_evaluation(dataset_dir=dataset_dir, traj_path=os.path.join(root, "traj.npy"), ply_path=os.path.join(root, "mesh.ply"), out_dir=out,
                               view_crop=False)
    finally:
        sys.path.pop(0)
        for m in mods:
            sys.modules.pop(m, None)
    name = os.path.basename(dataset_dir)
    prf = np.loadtxt(os.path.join(out, name + ".prf_tau_plotstr.txt"))
    return {"prf": prf, "cum_source": np.loadtxt(os.path.join(out, name + ".precision.txt")), "cum_target": np.loadtxt(os.path.join(out, name + ".recall.txt")),
            "final": LOG["transforms"][-1], "scored": list(LOG["scored"]), "stages": list(LOG["stages"]), "crops": list(LOG["crops"]), "criteria": LOG["criteria"], "trajectory": LOG["trajectory"]}


def main():
    rec = []
    with tempfile.TemporaryDirectory() as root:
        d = write_dataset(root)
        for k, case in enumerate(S.CASES):
            r = run_reference(root, d, None if k == 0 else case)
            if k == 0:      # what the reference's positional call turns into under Open3D's signature
                assert r["criteria"] == S.CASES[0], r["criteria"]
            print(case, r["prf"], [(s["source"], s["target"], s["iterations"]) for s in r["stages"]], r["crops"])
            rec.append(r)
    # the final transform is not written by the reference: it is the matrix of the last PointCloud.transform call, the one
    # EvaluateHisto makes (evaluation.py:76)
    st = np.array([[[s["source"], s["target"], s["iterations"]] for s in r["stages"]] for r in rec], np.int64)
    np.savez(os.path.join(HERE, "ref_tnt.npz"), scene=json.dumps(S.FIXTURE), cases=json.dumps(S.CASES), ransac_seed=S.RANSAC_SEED,
             prf=np.array([r["prf"] for r in rec]), cum_source=np.array([r["cum_source"] for r in rec]),
             cum_target=np.array([r["cum_target"] for r in rec]), stage_sizes=st,
             stage_fit=np.array([[[s["fitness"], s["inlier_rmse"], s["threshold"]] for s in r["stages"]] for r in rec]),
             crops=np.array([r["crops"] for r in rec], np.int64), scored=np.array([r["scored"] for r in rec], np.int64), final=np.array([r["final"] for r in rec]),
             trajectory=np.array([r["trajectory"]["transformation"] for r in rec]),
             trajectory_fit=np.array([[r["trajectory"]["fitness"], r["trajectory"]["inlier_rmse"]] for r in rec]))


if __name__ == "__main__":
    main()
