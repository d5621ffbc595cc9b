"""Generate tests/golden/ref_metrics.npz by running the reference's own lpipsPyTorch.LPIPS('vgg'), utils.image_utils.psnr,
utils.loss_utils.ssim and metrics.py::evaluate on the seeded pairs of tests/metrics_scenes.py (METRICS.md §Pinning).

torchvision, which lpipsPyTorch and metrics.py import, does not exist here, and the real LPIPS weights would come from the network.  A
stand-in `torchvision` goes into sys.modules BEFORE lpipsPyTorch is imported: models.vgg16(weights=...) returns an object whose
`features` is the 31-module nn.Sequential (conv / ReLU / pool in the order 64 64 M 128 128 M 256 256 256 M 512 512 512 M 512 512 512 M)
filled with the seeded weights, and transforms.functional.to_tensor is uint8 / 255.  get_state_dict is replaced by a function that
returns the seeded tap weights under the keys LinLayers expects, BEFORE any LPIPS is constructed, and torch.hub.load_state_dict_from_url
is replaced by a function that raises: this script cannot reach the network.  metrics.py sends tensors to a GPU with .cuda(); here
Tensor.cuda is the identity, so the reference's evaluate runs in fp32 on the CPU.

The fixture therefore pins what the reference's Python decides: the z-score, which modules are tapped, the normalisation, the squared
difference, the 1x1 weights, the spatial mean, the sum, psnr, ssim and the JSON structure.  torchvision's layer order itself is restated
from recollection and pinned only by the reference's target_layers = [4, 9, 16, 23, 30] and n_channels_list, which agree with it.
The fixture holds arrays and JSON text only; no weights.

Runs only where the reference checkout (REF_ROOT, default ../../../reference relative to this file) exists.
    python tests/golden/make_golden_metrics.py            writes ref_metrics.npz
"""
import contextlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn as nn

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
REF = os.path.abspath(os.environ.get("REF_ROOT", os.path.join(REPO, "..", "reference")))
sys.path.insert(0, os.path.join(REPO, "tests"))
import metrics_oracle as O  # noqa: E402
import metrics_scenes as S  # noqa: E402


# ---- no network: before anything of the reference is imported
def _no_network(*a, **k):
    raise RuntimeError("make_golden_metrics: a download was attempted")


torch.hub.load_state_dict_from_url = _no_network
torch.hub.download_url_to_file = _no_network


# ---- stand-in torchvision
def _vgg16(weights=None, **kw):
    convs, biases, _ = S.weights()
    cfg = [64, 64, "M", 128, 128, "M", 256, 256, 256, "M", 512, 512, 512, "M", 512, 512, 512, "M"]
    mods, cin, k = [], 3, 0
    for v in cfg:
        if v == "M":
            mods.append(nn.MaxPool2d(kernel_size=2, stride=2))
            continue
        conv = nn.Conv2d(cin, v, kernel_size=3, padding=1)
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(convs[k]))
            conv.bias.copy_(torch.from_numpy(biases[k]))
        mods += [conv, nn.ReLU(inplace=True)]
        cin, k = v, k + 1
    net = types.SimpleNamespace(features=nn.Sequential(*mods))
    assert len(net.features) == 31 and [i for i, m in enumerate(net.features) if isinstance(m, nn.Conv2d)] == list(S.CONV_INDEX)
    return net


def _to_tensor(pic):
    a = np.asarray(pic)
    assert a.dtype == np.uint8
    if a.ndim == 2:
        a = a[:, :, None]
    return torch.from_numpy(a.copy()).permute(2, 0, 1).contiguous().float().div(255)


tv = types.ModuleType("torchvision")
tv.models = types.ModuleType("torchvision.models")
tv.models.vgg16 = _vgg16
tv.models.VGG16_Weights = types.SimpleNamespace(IMAGENET1K_V1="IMAGENET1K_V1")
tv.transforms = types.ModuleType("torchvision.transforms")
tv.transforms.functional = types.ModuleType("torchvision.transforms.functional")
tv.transforms.functional.to_tensor = _to_tensor
for name, mod in (("torchvision", tv), ("torchvision.models", tv.models), ("torchvision.transforms", tv.transforms),
                  ("torchvision.transforms.functional", tv.transforms.functional)):
    sys.modules[name] = mod
for name in ("tqdm", "matplotlib", "matplotlib.pyplot"):      # imported by metrics.py / image_utils.py, not used by what runs here
    try:
        __import__(name)
    except ImportError:
        sys.modules[name] = types.ModuleType(name)
        if name == "tqdm":
            sys.modules[name].tqdm = lambda it, **k: it
        if name == "matplotlib":
            sys.modules[name].pyplot = None

sys.path.insert(0, REF)
import lpipsPyTorch.modules.lpips as ref_lpips_module  # noqa: E402
import lpipsPyTorch.modules.utils as ref_lpips_utils  # noqa: E402


def _seeded_state_dict(net_type="vgg", version="0.1"):
    assert net_type == "vgg"
    return {"%d.1.weight" % k: torch.from_numpy(l) for k, l in enumerate(S.weights()[2])}


ref_lpips_module.get_state_dict = _seeded_state_dict
ref_lpips_utils.get_state_dict = _seeded_state_dict

from lpipsPyTorch import lpips as ref_lpips  # noqa: E402,F401
from lpipsPyTorch.modules.lpips import LPIPS as RefLPIPS  # noqa: E402
from utils.image_utils import psnr as ref_psnr  # noqa: E402
from utils.loss_utils import ssim as ref_ssim  # noqa: E402


def main():
    model = RefLPIPS("vgg").double().eval()
    out = {"checksum": S.checksum(), "pairs": json.dumps(list(S.PAIRS)), "method": S.METHOD}
    lp, terms, ps, ss, ms, e32 = [], [], [], [], [], []
    with torch.no_grad():
        for k in range(len(S.PAIRS)):
            r, g = (torch.from_numpy(a).double().unsqueeze(0) for a in S.pair(k))
            lp.append(float(model(r, g)))
            assert tuple(model(r, g).shape) == (1, 1, 1, 1)
            # the per-layer terms: lpips.py:31-34 with the reference's own modules
            fx, fy = model.net(r), model.net(g)
            terms.append([float(l((a - b) ** 2).mean((2, 3), True)) for a, b, l in zip(fx, fy, model.lin)])
            ps.append(float(ref_psnr(r, g)))
            ms.append(float(((r - g) ** 2).view(1, -1).mean(1)))
            ss.append(float(ref_ssim(r, g)))
            o64 = O.lpips(r, g, S.weights(), torch.float64)
            o32 = O.lpips(r, g, S.weights(), torch.float32)
            rel = lambda a, b: abs(float(a) - float(b)) / abs(float(b))
            e32.append([rel(o32["terms"][j], o64["terms"][j]) for j in range(5)] + [rel(o32["total"], o64["total"])])
    out.update(lpips=np.array(lp), terms=np.array(terms), psnr=np.array(ps), mse=np.array(ms), ssim=np.array(ss), e32=np.array(e32))

    # metrics.py::evaluate (fp32, CPU) on a directory of the pairs' PNGs
    from PIL import Image
    torch.Tensor.cuda = lambda self, *a, **k: self
    import metrics as ref_metrics
    with tempfile.TemporaryDirectory() as tmp:
        scene = os.path.join(tmp, "scene")
        for sub in ("renders", "gt"):
            os.makedirs(os.path.join(scene, "test", S.METHOD, sub))
        for k, p in enumerate(S.PAIRS):
            for a, sub in zip(S.pair(k), ("renders", "gt")):
                u8 = np.round(a.transpose(1, 2, 0) * 255).astype(np.uint8)
                Image.fromarray(u8).save(os.path.join(scene, "test", S.METHOD, sub, p["name"]), "PNG")
        with contextlib.redirect_stdout(io.StringIO()) as log, contextlib.redirect_stderr(io.StringIO()):
            ref_metrics.evaluate([scene])
        assert "Unable" not in log.getvalue(), log.getvalue()
        out["results_json"] = open(os.path.join(scene, "results.json")).read()
        out["per_view_json"] = open(os.path.join(scene, "per_view.json")).read()
    path = os.path.join(HERE, "ref_metrics.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print("lpips", lp, "psnr", ps, "ssim", ss)
    print("e32", np.array(e32))
    print(out["results_json"])


if __name__ == "__main__":
    main()
