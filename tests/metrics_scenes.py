"""Seeded inputs of the image-quality tests (METRICS.md §Pinning): VGG16-shaped weights, LPIPS tap weights and two image pairs.
Everything is regenerated from seeds (numpy's RandomState stream) and nothing is stored; tests/golden/ref_metrics.npz keeps a checksum
of the weights so that a drift of the stream fails loudly instead of as a parity miss."""
import numpy as np

CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
            (512, 512), (512, 512), (512, 512))
TAP_CHANNELS = (64, 128, 256, 512, 512)
WEIGHT_SEED = 20241
PAIRS = ({"name": "00000.png", "H": 37, "W": 53, "seed": 7, "shift": (1, 2), "dim": 0.9},
         {"name": "00001.png", "H": 64, "W": 96, "seed": 8, "shift": (2, 1), "dim": 0.8})
METHOD = "ours_7"
SAMPLES = 5      # values per tensor in the checksum

_cache = {}


def weights():
    """(convs [C_out,C_in,3,3] x 13, biases [C_out] x 13, lins [1,C,1,1] x 5) as fp32 numpy arrays: He-normal, uniform +-0.1,
    uniform [0, 2/C).  Computed once; callers must not modify them."""
    if "w" not in _cache:
        rng = np.random.RandomState(WEIGHT_SEED)
        convs, biases, lins = [], [], []
        for cin, cout in CHANNELS:
            convs.append((rng.standard_normal((cout, cin, 3, 3)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32))
            biases.append(rng.uniform(-0.1, 0.1, cout).astype(np.float32))
        for c in TAP_CHANNELS:
            lins.append((rng.uniform(0.0, 2.0 / c, c)).astype(np.float32).reshape(1, c, 1, 1))
        _cache["w"] = (convs, biases, lins)
    return _cache["w"]


def checksum(tensors=None):
    """[n_tensors, 1 + SAMPLES] fp64: the sum of every tensor and SAMPLES values at fixed strides."""
    convs, biases, lins = tensors or weights()
    rows = []
    for t in list(convs) + list(biases) + list(lins):
        flat = np.asarray(t, np.float64).ravel()
        rows.append([flat.sum()] + [flat[(k * 7919) % flat.size] for k in range(SAMPLES)])
    return np.array(rows, np.float64)


def pair(k):
    """(render, gt) of pair k as [3, H, W] fp32 in [0, 1], every value a multiple of 1/255: structure plus noise; the render is the
    gt shifted, dimmed and noised again."""
    p = PAIRS[k]
    H, W = p["H"], p["W"]
    rng = np.random.RandomState(p["seed"])
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    base = np.stack([0.5 + 0.35 * np.sin(xx / 5.0 + c) * np.cos(yy / 7.0 - c) + 0.1 * ((xx // 8 + yy // 8) % 2) for c in range(3)])
    gt = np.clip(base + rng.normal(0, 0.05, base.shape), 0, 1)
    dy, dx = p["shift"]
    render = np.clip(np.roll(gt, (dy, dx), (1, 2)) * p["dim"] + rng.normal(0, 0.02, base.shape), 0, 1)
    q = lambda a: (np.round(a * 255).astype(np.uint8).astype(np.float32) / np.float32(255))
    return q(render), q(gt)


def state_dicts(prefix="features.", lin_style="lpips"):
    """The seeded weights under the key spellings surfel_metrics.load_lpips_weights accepts, as torch tensors."""
    import torch
    convs, biases, lins = weights()
    vgg = {}
    for i, w, b in zip(CONV_INDEX, convs, biases):
        vgg["%s%d.weight" % (prefix, i)] = torch.from_numpy(w)
        vgg["%s%d.bias" % (prefix, i)] = torch.from_numpy(b)
    name = "lin%d.model.1.weight" if lin_style == "lpips" else "%d.1.weight"
    lin = {name % k: torch.from_numpy(l) for k, l in enumerate(lins)}
    return vgg, lin
