"""Lift 2D label masks to per-surfel labels and split a model by them (SELECT.md).

Nothing of the reference is replaced: it has no segmentation.  The rule is FlashSplat's ("2D to 3D Gaussian splatting segmentation solved
optimally"): under linear blending the optimal label of a surfel is the arg-max, over the labels k, of the blend weight alpha * T it
contributes to the pixels whose mask says k, summed over all views.  The sums (votes) are accumulated by ONE HIP pass per view behind
the forward (include/surfel_select.h); the arg-max, the split and the files are torch plumbing on integers.

    python surfel_select.py -m MODEL_DIR [-s CAPTURE] [--iteration N] --masks DIR [--binary] [--num_labels K] (--keep K... | --remove K...)
                            [--bias B...] [--min_share S] [--report] [--out PLY] [--as_model DIR]
"""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

import surfel_native as _n

WHO = "surfel_select"
FRAC_BITS = 24                # include/surfel_select.h: SURFEL_SELECT_FRAC_BITS
MAX_LABELS = 32               # SURFEL_SELECT_MAX_LABELS
UNLABELLED = 255              # SURFEL_SELECT_UNLABELLED: any label >= K is ignored; this one says so by convention
launches = 0                  # label-pass launches of this process


class LabelVotes:
    """votes: int64 [P, K] — the library's unsigned sums held in torch's signed type of the same width (they stay far below the sign
    bit).  Integers, so adding views in any order gives the same bytes.  On a HIP device views can be added; on the CPU (load) the votes
    can be read, assigned and saved."""

    def __init__(self, P, K, device="cuda"):
        if int(P) < 0:
            raise ValueError("%s: P must not be negative" % WHO)
        if not 1 <= int(K) <= MAX_LABELS:
            raise ValueError("%s: the number of labels must be in 1 .. %d, got %d" % (WHO, MAX_LABELS, int(K)))
        self.P, self.K, self.device = int(P), int(K), torch.device(device)
        self.votes = torch.zeros((self.P, self.K), dtype=torch.int64, device=self.device)
        self.views = 0            # views added
        self.skipped = 0          # label_votes: cameras without a mask

    def add_view(self, buffers, labels):
        """Add the view whose forward left `buffers` (surfel_render.rasterize_buffers' dict, or a render package that carries it under
        "buffers": geom, binning, image, num_rendered, width, height, of a frame rendered with OPT_EXACT_BINNING) with its label image:
        a contiguous uint8 [H, W] tensor on the votes' device; a pixel whose label is >= K (by convention 255) votes for nothing."""
        global launches
        b, W, H = _n.view_buffers(WHO, buffers, self.device, self.P, "votes")
        _n.device_tensor(WHO, labels, "labels")
        if labels.dtype != torch.uint8:
            raise ValueError("%s: labels must be uint8, got %s" % (WHO, labels.dtype))
        if tuple(labels.shape) != (H, W):
            raise ValueError("%s: labels must be [%d, %d] (the view's height and width), got %s" % (WHO, H, W, list(labels.shape)))
        if labels.device != self.votes.device:
            raise ValueError("%s: labels live on %s, the votes on %s" % (WHO, labels.device, self.votes.device))
        labels = labels.contiguous()
        _n.call(self.device, "surfel_rasterize_label_votes", self.P, int(b["num_rendered"]), W, H, b["geom"], b["binning"], b["image"],
                labels, self.K, self.votes, 0)
        launches += 1
        self.views += 1

    @property
    def weights(self):
        """float64 [P, K]: the summed blend weights (each rounded to 2^-24)"""
        return self.votes.to(torch.float64) / float(1 << FRAC_BITS)

    # ---- files
    def save(self, path, labels=None):
        """.npz: votes, num_labels, views and, where given, the surfels' labels (int32 [P])"""
        arrays = dict(votes=self.votes.cpu().numpy(), num_labels=np.int64(self.K), views=np.int64(self.views))
        if labels is not None:
            arrays["labels"] = torch.as_tensor(labels).cpu().numpy().astype(np.int32)
        with open(path, "wb") as f:      # (a file object: numpy appends no .npz to it)
            np.savez(f, **arrays)

    @classmethod
    def load(cls, path, device="cpu"):
        with np.load(path) as z:
            v = torch.from_numpy(z["votes"])
            K = int(z["num_labels"])
            if v.dtype != torch.int64 or v.ndim != 2 or v.shape[1] != K:
                raise ValueError("%s: %s holds votes %s %s, expected int64 [P, %d]" % (WHO, path, v.dtype, tuple(v.shape), K))
            c = cls(v.shape[0], K, device)
            c.votes = v.to(c.device)
            c.views = int(z["views"])
        return c


def _label_tensor(labels, device):
    """a label image (numpy or torch, any integer type holding 0 .. 255) as a contiguous uint8 tensor on `device`"""
    t = torch.as_tensor(labels)
    if t.dtype != torch.uint8:
        if t.dtype.is_floating_point or t.numel() and (int(t.min()) < 0 or int(t.max()) > 255):
            raise ValueError("%s: a label image holds integers in 0 .. 255" % WHO)
        t = t.to(torch.uint8)
    return t.to(device).contiguous()


def label_votes(model, cams, masks, K, pipe, background):
    """Render every camera that has a mask once (no gradient, exact binning) and run the label pass behind it.  masks: image_name ->
    label image [H, W].  Cameras without a mask are skipped and counted (LabelVotes.skipped)."""
    from surfel_render import rasterize_buffers
    lv = LabelVotes(model.P, K, model.device)
    for cam in cams:
        m = masks.get(cam.image_name)
        if m is None:
            lv.skipped += 1
            continue
        _, _, _, buffers = rasterize_buffers(cam, model, pipe, background, debug_bits=_n.OPT_EXACT_BINNING)
        lv.add_view(buffers, _label_tensor(m, model.device))
    return lv


def assign(votes, bias=None, min_share=0.0):
    """int32 [P] label per surfel from votes (a LabelVotes or an integer [P, K] tensor).  The exact rule (SELECT.md):
        score[p, k] = votes[p, k]                      (int64; bias None)
                    = bias[k] * float64(votes[p, k])   (bias given: K non-negative finite numbers, FlashSplat's background softening)
        label[p]    = the LOWEST k whose score equals the row's maximum
        label[p]    = -1 where the row's votes are all zero, or where float64(votes[p, label]) < min_share * float64(sum_k votes[p, k])
    The share is taken of the unbiased votes."""
    v = votes.votes if isinstance(votes, LabelVotes) else votes
    if not torch.is_tensor(v) or v.ndim != 2 or v.dtype.is_floating_point or v.shape[1] < 1:
        raise ValueError("%s: votes must be an integer [P, K] tensor" % WHO)
    v = v.to(torch.int64)
    P, K = v.shape
    if not 0.0 <= float(min_share) <= 1.0:
        raise ValueError("%s: min_share must be in [0, 1]" % WHO)
    if bias is None:
        score = v
    else:
        b = torch.as_tensor(bias, dtype=torch.float64).reshape(-1)
        if b.numel() != K or not bool(torch.isfinite(b).all()) or bool((b < 0).any()):
            raise ValueError("%s: bias must hold %d non-negative finite numbers" % (WHO, K))
        score = v.to(torch.float64) * b.to(v.device)[None, :]
    best = score.max(dim=1, keepdim=True).values
    ks = torch.arange(K, device=v.device, dtype=torch.int64)[None, :].expand(P, K)
    label = torch.where(score == best, ks, torch.full_like(ks, K)).min(dim=1).values      # the lowest k among the maxima
    total = v.sum(dim=1)
    won = v.gather(1, label[:, None]).squeeze(1)
    none = (total == 0) | (won.to(torch.float64) < float(min_share) * total.to(torch.float64))
    return torch.where(none, torch.full_like(label, -1), label).to(torch.int32)


def select_mask(labels, keep=None, remove=None):
    """bool [P]: True where the surfel stays — its label is in `keep`, or is not in `remove` (-1, no label, may be listed in either)"""
    if (keep is None) == (remove is None):
        raise ValueError("%s: give keep or remove, not both and not neither" % WHO)
    if not torch.is_tensor(labels) or labels.dtype.is_floating_point or labels.ndim != 1:
        raise ValueError("%s: labels must be an integer [P] tensor" % WHO)
    listed = torch.zeros_like(labels, dtype=torch.bool)
    for k in (keep if keep is not None else remove):
        listed |= labels == int(k)
    return listed if keep is not None else ~listed


def split_model(model, labels, keep=None, remove=None):
    """Keep the surfels whose label is in `keep`, or drop those whose label is in `remove`, through GaussianModel.prune_points (as
    surfel_prune.prune_model does).  Returns the number of surfels removed."""
    from surfel_prune import prune_model
    if not torch.is_tensor(labels) or labels.numel() != model.P:
        raise ValueError("%s: labels must be a tensor of the model's %d surfels" % (WHO, model.P))
    return prune_model(model, select_mask(labels.reshape(-1), keep, remove))


def label_image(model, cam, labels, K, pipe):
    """uint8 [H, W]: per pixel the label with the largest accumulated blend weight (a tie goes to the lowest label), 255 where no
    labelled surfel was composited.  The existing forward with one-hot colours over a black background, three labels per render."""
    from surfel_render import rasterize_buffers
    if not 1 <= int(K) <= MAX_LABELS:
        raise ValueError("%s: the number of labels must be in 1 .. %d, got %d" % (WHO, MAX_LABELS, int(K)))
    if not torch.is_tensor(labels) or labels.numel() != model.P:
        raise ValueError("%s: labels must be a tensor of the model's %d surfels" % (WHO, model.P))
    dev = model.device
    lab = labels.reshape(-1).to(dev).to(torch.int64)
    black = torch.zeros(3, dtype=torch.float32, device=dev)
    maps = []
    for k0 in range(0, int(K), 3):
        onehot = torch.stack([(lab == k).to(torch.float32) for k in range(k0, k0 + 3)], dim=1).contiguous()      # (a label >= K: a zero column)
        image = rasterize_buffers(cam, model, pipe, black, override_color=onehot)[0]
        maps.append(image[:min(3, int(K) - k0)])
    acc = torch.cat(maps, dim=0)                      # [K, H, W]
    best = acc.max(dim=0, keepdim=True).values
    ks = torch.arange(int(K), device=dev, dtype=torch.int64)[:, None, None].expand_as(acc)
    out = torch.where(acc == best, ks, torch.full_like(ks, int(K))).min(dim=0).values
    return torch.where(best[0] > 0, out, torch.full_like(out, UNLABELLED)).to(torch.uint8)


# ------------------------------------------------------------------------------------------------ masks
def read_mask(path, width, height, binary=False):
    """The label image of one mask file (Pillow): 8-bit gray ("L") or palette ("P") — the pixel value (the palette index) is the label;
    binary: values above 127 become 1, the rest 0 (any other mode is read as gray first).  Resized to width x height with nearest
    neighbour.  Returns a uint8 [height, width] numpy array."""
    from PIL import Image
    with Image.open(path) as im:
        if im.mode not in ("L", "P"):
            if not binary:
                raise ValueError("%s: %s is a %s image; labels are read from 8-bit gray or palette images (or pass --binary)" % (WHO, path, im.mode))
            im = im.convert("L")
        if im.size != (int(width), int(height)):
            im = im.resize((int(width), int(height)), Image.NEAREST)
        a = np.array(im, dtype=np.uint8)
    if binary:
        a = (a > 127).astype(np.uint8)
    return np.ascontiguousarray(a)


def load_masks(folder, cams, binary=False):
    """({image_name: uint8 [H, W]}, names of the cameras without FOLDER/<image_name>.png)"""
    masks, missing = {}, []
    for cam in cams:
        p = os.path.join(folder, cam.image_name + ".png")
        if not os.path.exists(p):
            missing.append(cam.image_name)
            continue
        masks[cam.image_name] = read_mask(p, cam.image_width, cam.image_height, binary)
    return masks, missing


def report(model, cams, masks, lv, labels, pipe, out=print):
    """Per label: surfels, vote mass, and the IoU of label_image against the input masks, view by view"""
    lab = labels.cpu().numpy()
    mass = lv.weights.sum(0).cpu().numpy()
    out("%d surfels, %d labels over %d views (%d cameras without a mask): %d without a label" % (lv.P, lv.K, lv.views, lv.skipped, int((lab < 0).sum())))
    ious = {k: [] for k in range(lv.K)}
    for cam in cams:
        m = masks.get(cam.image_name)
        if m is None:
            continue
        got = label_image(model, cam, labels, lv.K, pipe).cpu().numpy()
        want = np.asarray(m)
        for k in range(lv.K):
            union = int(((got == k) | (want == k)).sum())
            if union:
                ious[k].append(int(((got == k) & (want == k)).sum()) / union)
    for k in range(lv.K):
        v = ious[k]
        out("  label %d: %d surfels, vote mass %.1f, IoU per view %s" % (k, int((lab == k).sum()), float(mass[k]),
                                                                         "-" if not v else "mean %.3f min %.3f [%s]" % (sum(v) / len(v), min(v), " ".join("%.3f" % x for x in v))))


def write_model_dir(folder, source_model, cams, gaussians, iteration):
    """A model directory surfel_mesh.py -m and surfel_view.py -m open: cfg_args (the source model's, pointed at `folder`),
    cameras.json (the source model's, or the cameras' own) and point_cloud/iteration_N/point_cloud.ply"""
    os.makedirs(folder, exist_ok=True)
    cfg = argparse.Namespace(sh_degree=gaussians.max_sh_degree, source_path="", images="images", resolution=-1, white_background=False,
                             data_device="cuda", eval=False)
    src = os.path.join(source_model, "cfg_args")
    if os.path.exists(src):
        cfg = eval(open(src).read(), {"Namespace": argparse.Namespace, "__builtins__": {}})
    cfg.model_path = folder
    with open(os.path.join(folder, "cfg_args"), "w") as f:
        f.write(str(cfg))
    src = os.path.join(source_model, "cameras.json")
    if os.path.exists(src):
        entries = json.load(open(src))
    else:      # read_cameras_json's inverse: position / rotation = camera-to-world, fx / fy in pixels
        entries = []
        for i, cam in enumerate(cams):
            R = np.asarray(cam.R, np.float64)
            W, H = int(cam.image_width), int(cam.image_height)
            entries.append({"id": i, "img_name": cam.image_name, "width": W, "height": H, "position": (-R @ np.asarray(cam.T, np.float64)).tolist(),
                            "rotation": [row.tolist() for row in R], "fy": H / (2 * math.tan(cam.FoVy / 2)), "fx": W / (2 * math.tan(cam.FoVx / 2))})
    with open(os.path.join(folder, "cameras.json"), "w") as f:
        json.dump(entries, f)
    pc = os.path.join(folder, "point_cloud", "iteration_%d" % iteration)
    os.makedirs(pc, exist_ok=True)
    gaussians.save_ply(os.path.join(pc, "point_cloud.ply"))
    return folder


# ------------------------------------------------------------------------------------------------ CLI
def build_parser():
    ap = argparse.ArgumentParser(description="Select the surfels of a trained model that 2D label masks point at (SELECT.md)")
    ap.add_argument("-m", "--model_path", type=str, required=True, help="the model directory (cameras.json, point_cloud/)")
    ap.add_argument("-s", "--source_path", type=str, default=None, help="the capture: its training cameras instead of cameras.json")
    ap.add_argument("--iteration", type=int, default=-1)
    ap.add_argument("--masks", type=str, required=True, help="DIR/<image_name>.png: 8-bit gray or palette, the pixel value is the label (255: none)")
    ap.add_argument("--binary", action="store_true", help="mask values above 127 are label 1, the rest label 0")
    ap.add_argument("--num_labels", type=int, default=None, help="K, 1 .. 32 (default: 2 with --binary, else the largest label below 255 seen, plus one)")
    sel = ap.add_mutually_exclusive_group()
    sel.add_argument("--keep", type=int, nargs="+", default=None, help="keep the surfels with these labels (-1: those without a label)")
    sel.add_argument("--remove", type=int, nargs="+", default=None, help="remove the surfels with these labels")
    ap.add_argument("--bias", type=float, nargs="+", default=None, help="K factors on the votes before the arg-max (default: all ones)")
    ap.add_argument("--min_share", type=float, default=0.0, help="a surfel whose winning label holds less than this share of its votes gets none")
    ap.add_argument("--white_background", action="store_true")
    ap.add_argument("--report", action="store_true", help="print per label the surfels, the vote mass and the IoU of the re-rendered labels; write nothing")
    ap.add_argument("--out", type=str, default=None, help="the selected .ply (default point_cloud/iteration_N/point_cloud_selected.ply)")
    ap.add_argument("--as_model", type=str, default=None, help="also write a model directory with the selection (cfg_args, cameras.json, point_cloud/)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if not args.report and args.keep is None and args.remove is None:
        raise SystemExit("give --keep or --remove (or --report)")
    import surfel_mesh
    gaussians, cams, it, folder, pipe, bg = surfel_mesh.open_model(args, torch.device("cuda:0"))
    masks, missing = load_masks(args.masks, cams, args.binary)
    if not masks:
        raise SystemExit("no mask under %s matches a camera's image name" % args.masks)
    K = args.num_labels
    if K is None:
        K = 2 if args.binary else 1 + max(int(m[m != UNLABELLED].max(initial=0)) for m in masks.values())
    lv = label_votes(gaussians, cams, masks, K, pipe, bg)
    labels = assign(lv, bias=args.bias, min_share=args.min_share)
    if args.report:
        report(gaussians, cams, masks, lv, labels, pipe)
        return 0
    lv.save(os.path.join(folder, "labels.npz"), labels=labels)
    removed = split_model(gaussians, labels, keep=args.keep, remove=args.remove)
    out = args.out or os.path.join(folder, "point_cloud_selected.ply")
    gaussians.save_ply(out)
    if args.as_model:
        write_model_dir(args.as_model, args.model_path, cams, gaussians, it)
    print("%d of %d surfels removed over %d views (%d cameras without a mask) -> %s" % (removed, lv.P, lv.views, len(missing), out))
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
