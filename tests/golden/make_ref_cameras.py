"""Generate tests/golden/ref_cameras.json with the reference's own camera_to_JSON (utils/camera_utils.py:64-84) and, next to it,
ref_cameras_source.json: the R, T, FoV and image size each entry was made from.

Runs only where the reference checkout exists (REF_ROOT, default ../../../reference relative to this file); the two JSON files it
writes are committed."""
import json
import os
import sys

import numpy as np

REF = os.environ.get("REF_ROOT", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..", "..", "reference"))
sys.path.insert(0, REF)
import types  # noqa: E402
# camera_utils imports the reference's scene package (plyfile, the CUDA knn extension): stand in for the two names it takes from there
for _name, _attrs in (("scene", {}), ("scene.cameras", {"Camera": object})):
    _mod = types.ModuleType(_name)
    _mod.__dict__.update(_attrs)
    sys.modules.setdefault(_name, _mod)
from utils.camera_utils import camera_to_JSON  # noqa: E402


class Cam:
    def __init__(self, R, T, fovx, fovy, w, h, name):
        self.R, self.T, self.FovX, self.FovY, self.width, self.height, self.image_name = R, T, fovx, fovy, w, h, name


def main():
    rng = np.random.default_rng(7)
    entries, source = [], []
    for k in range(3):
        q = rng.normal(size=4); q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        T = rng.normal(size=3) * 2.0
        W, H = [(64, 48), (100, 75), (33, 20)][k]
        fovx, fovy = 0.8 + 0.1 * k, 0.6 + 0.05 * k
        entries.append(camera_to_JSON(k, Cam(R, T, fovx, fovy, W, H, "view_%02d" % k)))
        source.append({"R": R.tolist(), "T": T.tolist(), "FoVx": fovx, "FoVy": fovy, "width": W, "height": H})
    here = os.path.dirname(os.path.abspath(__file__))
    json.dump(entries, open(os.path.join(here, "ref_cameras.json"), "w"))
    json.dump(source, open(os.path.join(here, "ref_cameras_source.json"), "w"))


if __name__ == "__main__":
    main()
