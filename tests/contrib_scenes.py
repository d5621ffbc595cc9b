"""The scenes of the contribution tests (tests/test_contrib_cpu.py, tests/test_gpu_contrib.py) — TEST INFRASTRUCTURE.

Each entry returns (scene dict, colors_precomp or None, n_theta of the oracle's bounding-box sampling).  The seeds are chosen on the CPU
(test_contrib_cpu.test_gpu_scenes_are_determined): at most 1 % of the covered pixels of every scene may be undetermined.
"""
import numpy as np

import analytic


def random_scene(seed, P, W=72, H=56, view_index=0):
    """tilted random surfels as tests/test_gpu_analytic.py::test_hip_matches_ray_plane_renderer builds them; 72 x 56 = 5 x 4 tiles, partial
    on both edges"""
    import synthetic
    sc = synthetic.make_scene(P, W, H, seed=seed, px_radius=7.0, z_near=2.0, z_far=7.0, tilt=True, view_index=view_index)
    rng = np.random.default_rng(seed)
    sc["bg"] = np.array([0.3, 0.1, 0.6], np.float32)
    sc["opacities"] = rng.uniform(0.05, 0.95, (P, 1)).astype(np.float32)
    cols = rng.uniform(0, 1, (P, 3)).astype(np.float32)
    return sc, cols, 200_000


def stacked_scene(o1):
    """the discs of test_hip_two_stacked_discs: the big one spans all 16 tiles of 64 x 64"""
    return analytic.axis_scene(64, 64, [(2.5, 0.10, 0.10, o1, (1.0, 0.1, 0.1)), (6.0, 0.40, 0.30, 0.9, (0.1, 0.2, 1.0))]), None, 200_000


def tiny_scene():
    """the disc of test_hip_tiny_disc_low_pass"""
    sc = analytic.axis_scene(48, 48, [(4.0, 0.004, 0.003, 0.9, (0.2, 0.7, 0.5))], bg=(0.0, 0.0, 0.0))
    sc["means3D"][0, :2] = [0.013, -0.021]
    return sc, None, 200_000


LONG_P = 700


LONG_FAINT = 300


def long_scene(seed=3):
    """700 large discs stacked along the axis of a 48 x 48 frame: every one of the 9 tile lists holds all of them (three staging
    batches).  The nearest 300 are faint (alpha 0.6 - 0.8 %, clear of the 1/255 threshold) and leave T near 0.12; the rest have high
    opacity (0.4 - 0.6), so every pixel saturates (T < 1e-4) a dozen surfels into them: inside the second batch, in steps of a factor
    two (a crossing within 1e-3 of the threshold is rare, which long runs of faint surfels alone would not give)"""
    rng = np.random.default_rng(seed)
    z = np.sort(rng.uniform(2.0, 9.0, LONG_P))
    opa = np.where(np.arange(LONG_P) < LONG_FAINT, rng.uniform(0.006, 0.008, LONG_P), rng.uniform(0.4, 0.6, LONG_P))
    size = np.where(np.arange(LONG_P) < LONG_FAINT, 15.0, 4.0)      # the dense discs fall off towards the frame's corners: pixels saturate at different depths
    discs = [(float(z[k]), float(size[k]), float(size[k]), float(opa[k]), tuple(rng.uniform(0, 1, 3))) for k in range(LONG_P)]
    sc = analytic.axis_scene(48, 48, discs)
    return sc, None, 2_000


ORACLE_SCENES = {
    "random14": lambda: random_scene(1, 14),
    "random40": lambda: random_scene(6, 40),
    "stacked035": lambda: stacked_scene(0.35),
    "stacked085": lambda: stacked_scene(0.85),
    "tiny": tiny_scene,
    "long": long_scene,
}


def colors_of(sc, cols):
    """the colours a scene is rendered with through colors_precomp (its own SH base colours where the scene brings none)"""
    return np.ascontiguousarray(sc["_rgb"] if cols is None else cols, np.float32)
