"""Image-quality evaluation of held-out views on MI355X — the counterpart of the reference's metrics.py (METRICS.md).

    psnr(img1, img2)            utils/image_utils.py:19-21, [B,1]
    ssim                        surfel_losses.ssim (utils/loss_utils.py:43-73)
    LPIPS(weights)(x, y)        lpipsPyTorch.LPIPS('vgg').forward, [1,1,1,1]; .layers(x, y): the five layer terms
    evaluate(model_paths, weights)   metrics.py:36-92: MODEL/test/*/{renders,gt}/*.png -> results.json, per_view.json

The VGG16 feature stack runs as HIP kernels of libsurfel_hip.so (include/surfel_metrics.h): f32-input MFMA convolutions, pool, tap and
fixed-order partial sums; torch carves the workspace and holds the weights.  No CPU / PyTorch fallback: CPU tensors raise.  Weights are
read from files the caller names; nothing here fetches anything.
"""
import argparse
import json
import os
import sys

import torch

import surfel_native as _n
from surfel_losses import ssim  # noqa: F401  (re-export)

# torchvision's vgg16().features: the 13 convolutions' module indices and (C_in, C_out); a pool follows the convolutions listed in POOL_AFTER
# and a tap the ones in TAP_AFTER (relu1_2, relu2_2, relu3_3, relu4_3, relu5_3 = modules 4, 9, 16, 23, 30 counted from 1).
CONV_INDEX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
CHANNELS = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
            (512, 512), (512, 512), (512, 512))
TAP_AFTER = (1, 3, 6, 9, 12)
POOL_AFTER = (1, 3, 6, 9)
TAP_CHANNELS = (64, 128, 256, 512, 512)
MIN_EDGE = 16
DEFAULT_BUDGET = 16 << 30
NPART = 1024      # SURFEL_METRICS_PARTIALS
LimitError = _n.LimitError


def _device_image(t, what):
    if not isinstance(t, torch.Tensor) or t.device.type != "cuda":
        raise RuntimeError("surfel_metrics: tensors must live on a HIP device (got %s for %s)" % (getattr(t, "device", type(t)), what))
    return t.detach().contiguous().float()


def mse(img1, img2):
    """mean squared error per batch element over everything else (utils/image_utils.py:16-17): [B,1]."""
    if img1.shape != img2.shape or img1.dim() < 2:
        raise ValueError("image shapes differ: %s vs %s" % (tuple(img1.shape), tuple(img2.shape)))
    a, b = _device_image(img1, "img1"), _device_image(img2, "img2")
    dev, B = a.device, int(a.shape[0])
    n = a.numel() // B
    a, b = a.view(B, n), b.view(B, n)
    partials = torch.empty((B, NPART), dtype=torch.float32, device=dev)
    out = torch.empty((B,), dtype=torch.float32, device=dev)
    for k in range(B):
        _n.call(dev, "surfel_sq_err_partials", n, a[k], b[k], partials[k])
    _n.call(dev, "surfel_reduce_partials", partials, B, NPART, 1, 1.0 / n, out)
    return out.view(B, 1)


def psnr(img1, img2):
    """20 log10(1 / sqrt(mse)) (utils/image_utils.py:19-21): [B,1]."""
    return 20 * torch.log10(1.0 / torch.sqrt(mse(img1, img2)))


# ------------------------------------------------------------------------------------------------ weights
class LPIPSWeights:
    """13 convolution weights as [9, C_in (3 padded to 4), C_out] (tap-major, C_out contiguous), 13 biases, 5 tap weights [C]."""

    def __init__(self, convs, biases, lins):
        self.convs, self.biases, self.lins = convs, biases, lins

    def to(self, device):
        f = lambda ts: [t.to(device) for t in ts]
        return LPIPSWeights(f(self.convs), f(self.biases), f(self.lins))


def lpips_weights_from_tensors(convs, biases, lins):
    """convs: 13 tensors [C_out, C_in, 3, 3] in torchvision's order; biases: 13 [C_out]; lins: 5 [1, C, 1, 1] or [C]."""
    if len(convs) != 13 or len(biases) != 13 or len(lins) != 5:
        raise ValueError("LPIPS-VGG needs 13 convolutions, 13 biases and 5 tap weights")
    cw, cb, cl = [], [], []
    for k, (w, b) in enumerate(zip(convs, biases)):
        cin, cout = CHANNELS[k]
        if tuple(w.shape) != (cout, cin, 3, 3) or tuple(b.shape) != (cout,):
            raise ValueError("convolution %d: expected weight %s and bias %s, got %s and %s" % (k, (cout, cin, 3, 3), (cout,), tuple(w.shape), tuple(b.shape)))
        t = w.detach().float().permute(2, 3, 1, 0).reshape(9, cin, cout)
        if cin == 3:
            t = torch.cat([t, torch.zeros((9, 1, cout), dtype=torch.float32, device=t.device)], 1)
        cw.append(t.contiguous())
        cb.append(b.detach().float().contiguous())
    for k, l in enumerate(lins):
        if l.numel() != TAP_CHANNELS[k]:
            raise ValueError("tap %d: expected %d weights, got %s" % (k, TAP_CHANNELS[k], tuple(l.shape)))
        cl.append(l.detach().float().reshape(-1).contiguous())
    return LPIPSWeights(cw, cb, cl)


def _pick(sd, names, path):
    for n in names:
        if n in sd:
            return sd[n]
    raise KeyError("%s: missing key %r" % (path, names[0]))


def load_lpips_weights(vgg16_path, lin_path):
    """vgg16_path: a torchvision vgg16 state dict (features.N.weight / .bias, or N.weight / .bias); lin_path: LPIPS v0.1 vgg.pth
    (linK.model.1.weight, or the reference's renamed K.1.weight, modules/utils.py:23-28).  Local files only."""
    vgg = torch.load(vgg16_path, map_location="cpu", weights_only=True)
    lin = torch.load(lin_path, map_location="cpu", weights_only=True)
    convs = [_pick(vgg, ("features.%d.weight" % i, "%d.weight" % i), vgg16_path) for i in CONV_INDEX]
    biases = [_pick(vgg, ("features.%d.bias" % i, "%d.bias" % i), vgg16_path) for i in CONV_INDEX]
    lins = [_pick(lin, ("lin%d.model.1.weight" % k, "%d.1.weight" % k), lin_path) for k in range(5)]
    return lpips_weights_from_tensors(convs, biases, lins)


# ------------------------------------------------------------------------------------------------ LPIPS
def workspace_bytes(H, W, budget_bytes=DEFAULT_BUDGET):
    """Bytes LPIPS needs for an H x W pair; LimitError when that exceeds budget_bytes (nothing is allocated)."""
    return int(_n.call(None, "surfel_lpips_workspace_bytes", int(H), int(W), int(budget_bytes)))


def conv3x3(act, weight, bias):
    """relu(conv3x3 + bias) of act [2,H,W,C_in] with weight [9,C_in,C_out] -> [2,H,W,C_out] (one layer; tests and the bench script)."""
    act = _device_image(act, "act")
    _, H, W, cin = act.shape
    out = torch.empty((2, H, W, weight.shape[2]), dtype=torch.float32, device=act.device)
    _n.call(act.device, "surfel_lpips_conv3x3", H, W, cin, int(weight.shape[2]), act, weight, bias, out)
    return out


def pool(act):
    """2 x 2 max-pool of act [2,H,W,C] -> [2,H//2,W//2,C]."""
    act = _device_image(act, "act")
    _, H, W, C = act.shape
    out = torch.empty((2, H // 2, W // 2, C), dtype=torch.float32, device=act.device)
    _n.call(act.device, "surfel_lpips_pool", H, W, C, act, out)
    return out


def tap(act, lin):
    """mean over pixels of sum_c lin_c (fx_c / (|fx| + 1e-10) - fy_c / (|fy| + 1e-10))^2 for act [2,H,W,C]: a [1] tensor."""
    act = _device_image(act, "act")
    _, H, W, C = act.shape
    partials = torch.empty((NPART,), dtype=torch.float32, device=act.device)
    out = torch.empty((1,), dtype=torch.float32, device=act.device)
    _n.call(act.device, "surfel_lpips_tap", H, W, C, act, lin, partials)
    _n.call(act.device, "surfel_reduce_partials", partials, 1, NPART, 1, 1.0 / (H * W), out)
    return out


class LPIPS:
    """LPIPS v0.1 with the VGG16 features, as lpipsPyTorch.LPIPS('vgg') computes it: inputs in [0, 1] go through the z-score as they
    are.  weights: LPIPSWeights (moved to `device`)."""

    def __init__(self, weights, device="cuda", budget_bytes=DEFAULT_BUDGET):
        self.device = torch.device(device)
        self.weights = weights.to(self.device)
        self.budget_bytes = int(budget_bytes)
        self.timings = None      # a dict: ms per stage of the next call (scripts/metrics_bench.py)

    def _pair(self, x, y):
        x, y = _device_image(x, "x"), _device_image(y, "y")
        if x.dim() == 4 and x.shape[0] == 1:
            x, y = x[0], y[0]
        if x.dim() != 3 or x.shape[0] != 3 or x.shape != y.shape:
            raise ValueError("LPIPS takes [1,3,H,W] or [3,H,W] pairs of one size, got %s and %s" % (tuple(x.shape), tuple(y.shape)))
        H, W = int(x.shape[1]), int(x.shape[2])
        if H < MIN_EDGE or W < MIN_EDGE:
            raise ValueError("LPIPS needs H, W >= %d (relu5_3 would be empty), got %d x %d" % (MIN_EDGE, H, W))
        return x, y, H, W

    def layers(self, x, y):
        """The five layer terms (relu1_2 .. relu5_3), a [5] tensor; LPIPS is their sum in this order."""
        x, y, H, W = self._pair(x, y)
        dev, w = x.device, self.weights
        nbytes = workspace_bytes(H, W, self.budget_bytes)      # LimitError before anything is allocated
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        act_bytes = (nbytes - 6 * NPART * 4) // 2
        buf = [ws[:act_bytes].view(torch.float32), ws[act_bytes:2 * act_bytes].view(torch.float32)]
        partials = ws[2 * act_bytes:].view(torch.float32).view(6, NPART)
        terms = torch.empty((5,), dtype=torch.float32, device=dev)
        t = _StageTimer(self.timings, dev)
        cur = 1
        _n.call(dev, "surfel_lpips_prepare", H, W, x, y, buf[cur])
        t.lap("prepare")
        tapped = 0
        for k, (cin, cout) in enumerate(CHANNELS):
            _n.call(dev, "surfel_lpips_conv3x3", H, W, max(cin, 4), cout, buf[cur], w.convs[k], w.biases[k], buf[1 - cur])
            cur = 1 - cur
            t.lap("conv%d" % k)
            if k in TAP_AFTER:
                _n.call(dev, "surfel_lpips_tap", H, W, cout, buf[cur], w.lins[tapped], partials[tapped])
                _n.call(dev, "surfel_reduce_partials", partials[tapped], 1, NPART, 1, 1.0 / (H * W), terms[tapped:tapped + 1])
                tapped += 1
                t.lap("tap")
            if k in POOL_AFTER:
                _n.call(dev, "surfel_lpips_pool", H, W, cout, buf[cur], buf[1 - cur])
                cur, H, W = 1 - cur, H // 2, W // 2
                t.lap("pool")
        return terms

    def __call__(self, x, y):
        terms = self.layers(x, y)
        total = terms[0]
        for k in range(1, 5):      # torch.sum(torch.cat(res, 0), 0): the five terms in layer order
            total = total + terms[k]
        return total.view(1, 1, 1, 1)


def lpips(x, y, weights):
    return LPIPS(weights, x.device)(x, y)


class _StageTimer:
    """ms per stage into a dict (synchronises at every lap); inert when the dict is None."""

    def __init__(self, sink, device):
        self.sink, self.device = sink, device
        if sink is not None:
            self.ev = torch.cuda.Event(enable_timing=True)
            self.ev.record()

    def lap(self, name):
        if self.sink is None:
            return
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        e.synchronize()
        self.sink[name] = self.sink.get(name, 0.0) + self.ev.elapsed_time(e)
        self.ev = e


# ------------------------------------------------------------------------------------------------ metrics.py
def read_image(path, device):
    """torchvision's to_tensor of a PNG: uint8 / 255 as [1, 3, H, W] (first three channels) on the device."""
    import numpy as np
    from PIL import Image
    a = np.asarray(Image.open(path))
    if a.dtype != np.uint8:
        raise ValueError("%s: expected an 8-bit image, got %s" % (path, a.dtype))
    if a.ndim == 2:
        a = a[:, :, None]
    t = torch.from_numpy(a.copy()).permute(2, 0, 1).float().div(255)
    return t.unsqueeze(0)[:, :3, :, :].to(device)


def read_images(renders_dir, gt_dir, device):
    renders, gts, names = [], [], []
    for fname in sorted(os.listdir(renders_dir)):
        renders.append(read_image(os.path.join(renders_dir, fname), device))
        gts.append(read_image(os.path.join(gt_dir, fname), device))
        names.append(fname)
    return renders, gts, names


def _mean(values):
    return torch.tensor(values).mean().item()


def evaluate(model_paths, weights=None, device="cuda"):
    """metrics.py:36-92.  For every scene and every MODEL/test/<method>/: SSIM, PSNR and LPIPS of renders/ against gt/, matched by file
    name in sorted order; writes MODEL/results.json and MODEL/per_view.json.  weights=None: "LPIPS" is null.  Returns (full, per_view)."""
    device = torch.device(device)
    criterion = None
    if weights is None:
        print("LPIPS: no weights given (--vgg16 and --lpips_lin), writing null; SSIM and PSNR are computed", file=sys.stderr)
    else:
        criterion = LPIPS(weights, device)
    full_dict, per_view_dict = {}, {}
    for scene_dir in model_paths:
        try:
            print("Scene:", scene_dir)
            full_dict[scene_dir], per_view_dict[scene_dir] = {}, {}
            test_dir = os.path.join(scene_dir, "test")
            for method in sorted(os.listdir(test_dir)):
                print("Method:", method)
                method_dir = os.path.join(test_dir, method)
                renders, gts, names = read_images(os.path.join(method_dir, "renders"), os.path.join(method_dir, "gt"), device)
                ssims, psnrs, lpipss = [], [], []
                for r, g in zip(renders, gts):
                    ssims.append(float(ssim(r, g)))
                    psnrs.append(float(psnr(r, g)))
                    if criterion is not None:
                        lpipss.append(float(criterion(r, g)))
                print("  SSIM : {:>12.7f}".format(_mean(ssims)))
                print("  PSNR : {:>12.7f}".format(_mean(psnrs)))
                print("  LPIPS: " + ("{:>12.7f}".format(_mean(lpipss)) if criterion is not None else "        null"))
                print("")
                full_dict[scene_dir][method] = {"SSIM": _mean(ssims), "PSNR": _mean(psnrs), "LPIPS": _mean(lpipss) if criterion is not None else None}
                per_view = lambda vals: {name: v for v, name in zip(torch.tensor(vals).tolist(), names)}
                per_view_dict[scene_dir][method] = {"SSIM": per_view(ssims), "PSNR": per_view(psnrs),
                                                    "LPIPS": per_view(lpipss) if criterion is not None else None}
            with open(os.path.join(scene_dir, "results.json"), "w") as fp:
                json.dump(full_dict[scene_dir], fp, indent=True)
            with open(os.path.join(scene_dir, "per_view.json"), "w") as fp:
                json.dump(per_view_dict[scene_dir], fp, indent=True)
        except Exception as e:      # (the reference's bare except hides the reason)
            print("Unable to compute metrics for model %s: %s: %s" % (scene_dir, type(e).__name__, e), file=sys.stderr)
    return full_dict, per_view_dict


def main(argv=None):
    ap = argparse.ArgumentParser(description="SSIM / PSNR / LPIPS-VGG of MODEL/test/*/renders against gt (the reference's metrics.py)")
    ap.add_argument("--model_paths", "-m", required=True, nargs="+", type=str, default=[])
    ap.add_argument("--vgg16", default=None, help="torchvision vgg16 state dict (a local file)")
    ap.add_argument("--lpips_lin", default=None, help="LPIPS v0.1 vgg.pth (a local file)")
    args = ap.parse_args(argv)
    weights = None
    if args.vgg16 and args.lpips_lin:
        weights = load_lpips_weights(args.vgg16, args.lpips_lin)
    elif args.vgg16 or args.lpips_lin:
        ap.error("--vgg16 and --lpips_lin go together")
    evaluate(args.model_paths, weights)
    return 0


if __name__ == "__main__":
    sys.exit(main())
