"""Score surfels by what they contribute to the blend and prune a model by it (CONTRIB.md).

Nothing of the reference is replaced: it prunes by opacity and screen size only, during densification (scene/gaussian_model.py,
mirrored in surfel_model.densify_and_prune).  The scores are LightGaussian's significance (the sum of blend weights), RadSplat's rule
(the maximum blend weight) and Mini-Splatting's count (the pixels a surfel dominates), accumulated over the training views by ONE HIP
pass per view behind the forward (include/surfel_contrib.h); ranking and masks are torch plumbing.

    python surfel_prune.py -m MODEL_DIR [-s CAPTURE] [--iteration N] [--min_max_weight T] [--min_views K] [--keep N | --keep_ratio R]
                           [--score sum|max|dominant] [--report] [--out PLY]
"""
import argparse
import os
import sys

import numpy as np
import torch

import surfel_native as _n

WHO = "surfel_prune"
FRAC_BITS = 24                # include/surfel_contrib.h: SURFEL_CONTRIB_FRAC_BITS
SCORES = ("sum", "max", "dominant")
_FIELDS = (("sum_q", torch.int64), ("hits_q", torch.int64), ("max_bits", torch.int32), ("dominant_q", torch.int32), ("views_q", torch.int32),
           ("stamp", torch.int32))
launches = 0                  # contribution launches of this process (tests: a run without the trainer's flags makes none)


class Contribution:
    """The six accumulator arrays of a model of P surfels.  They are integers (the unsigned arrays of the library held in torch's signed
    types of the same width: the counts stay far below the sign bit, and a positive float's bits are a positive int32), so adding views
    in any order gives the same bytes.  On a HIP device views can be added; on the CPU (load) it can be read, ranked and saved."""

    def __init__(self, P, device="cuda"):
        if int(P) < 0:
            raise ValueError("%s: P must not be negative" % WHO)
        self.P, self.device = int(P), torch.device(device)
        for name, dt in _FIELDS:
            setattr(self, name, torch.zeros(self.P, dtype=dt, device=self.device))
        self.next_tag = 1
        self.dominant_ids = []      # with add_view(..., dominant_id=True): this view's heaviest surfel per pixel [H, W] int32, -1 = none

    def add_view(self, buffers, tag=None, dominant_id=False):
        """Add the view whose forward left `buffers`: surfel_render.rasterize_buffers' dict (or a render package that carries it under
        "buffers") — geom, binning, image, num_rendered, width, height — of a frame rendered with OPT_EXACT_BINNING.  tag: the view's
        number, >= 1 and rising from call to call (default: the next one); a tag seen before counts no view twice."""
        global launches
        b, W, H = _n.view_buffers(WHO, buffers, self.device, self.P, "accumulators")
        tag = self.next_tag if tag is None else int(tag)
        if not 1 <= tag < 2 ** 31:
            raise ValueError("%s: tag must be in [1, 2^31)" % WHO)
        dom = torch.full((H, W), -1, dtype=torch.int32, device=self.device) if dominant_id else None
        _n.call(self.device, "surfel_rasterize_contribution", self.P, int(b["num_rendered"]), W, H, b["geom"], b["binning"], b["image"], tag,
                self.sum_q, self.hits_q, self.max_bits, self.dominant_q, self.views_q, self.stamp, dom, 0)
        launches += 1
        self.next_tag = max(self.next_tag, tag + 1)
        if dominant_id:
            self.dominant_ids.append(dom)
        return dom

    # ---- the statistics
    @property
    def sum_w(self):
        """float64 [P]: the sum of the blend weights (each rounded to 2^-24)"""
        return self.sum_q.to(torch.float64) / float(1 << FRAC_BITS)

    @property
    def max_w(self):
        """float32 [P]: the largest blend weight (0 where the surfel never composited)"""
        return self.max_bits.view(torch.float32)

    @property
    def hits(self):
        return self.hits_q

    @property
    def dominant(self):
        return self.dominant_q

    @property
    def views(self):
        return self.views_q

    # ---- files
    def save(self, path):
        arrays = {name: getattr(self, name).cpu().numpy() for name, _ in _FIELDS}
        with open(path, "wb") as f:      # (a file object: numpy appends no .npz to it)
            np.savez(f, next_tag=np.int64(self.next_tag), **arrays)

    @classmethod
    def load(cls, path, device="cpu"):
        with np.load(path) as z:
            c = cls(z["sum_q"].shape[0], device)
            for name, dt in _FIELDS:
                a = torch.from_numpy(z[name])
                if a.dtype != dt or a.shape != (c.P,):
                    raise ValueError("%s: %s holds %s %s of %s, expected %s [%d]" % (WHO, path, name, a.dtype, tuple(a.shape), dt, c.P))
                setattr(c, name, a.to(c.device))
            c.next_tag = int(z["next_tag"])
        return c


def contribution(model, cams, pipe, background, dominant_ids=False):
    """Render every camera once (no gradient, exact binning), run the contribution pass behind each, return the Contribution."""
    from surfel_render import rasterize_buffers
    c = Contribution(model.P, model.device)
    for cam in cams:
        _, _, _, buffers = rasterize_buffers(cam, model, pipe, background, debug_bits=_n.OPT_EXACT_BINNING)
        c.add_view(buffers, dominant_id=dominant_ids)
    return c


def _score_key(contrib, score):
    if score not in SCORES:
        raise ValueError("%s: score must be one of %s" % (WHO, ", ".join(SCORES)))
    # integer keys: the bits of a positive float order as the float does
    return {"sum": contrib.sum_q, "max": contrib.max_bits, "dominant": contrib.dominant_q}[score].to(torch.int64)


def prune_mask(contrib, *, min_max_weight=None, min_views=None, keep=None, keep_ratio=None, score="sum"):
    """bool [P] keep-mask: max_w >= min_max_weight AND views >= min_views AND among the `keep` (or keep_ratio * P, rounded down) best by
    `score`; a tie in the ranking goes to the lower surfel index.  A rule that is None does not restrict."""
    key = _score_key(contrib, score)
    if keep is not None and keep_ratio is not None:
        raise ValueError("%s: give keep or keep_ratio, not both" % WHO)
    if keep_ratio is not None:
        if not 0.0 <= float(keep_ratio) <= 1.0:
            raise ValueError("%s: keep_ratio must be in [0, 1]" % WHO)
        keep = int(float(keep_ratio) * contrib.P)
    if keep is not None and int(keep) < 0:
        raise ValueError("%s: keep must not be negative" % WHO)
    if min_views is not None and int(min_views) < 0:
        raise ValueError("%s: min_views must not be negative" % WHO)
    if min_max_weight is not None and not float(min_max_weight) >= 0.0:
        raise ValueError("%s: min_max_weight must not be negative" % WHO)
    mask = torch.ones(contrib.P, dtype=torch.bool, device=contrib.sum_q.device)
    if min_max_weight is not None:
        mask &= contrib.max_w >= float(min_max_weight)
    if min_views is not None:
        mask &= contrib.views >= int(min_views)
    if keep is not None and int(keep) < contrib.P:
        order = torch.sort(key, descending=True, stable=True).indices      # (stable: equal scores stay in index order)
        best = torch.zeros_like(mask)
        best[order[:int(keep)]] = True
        mask &= best
    return mask


def unseen_mask(contrib):
    """bool [P]: the surfels that neither composited nor terminated a pixel of any view added"""
    return contrib.views == 0


def prune_model(model, mask):
    """Keep the surfels where mask is True: GaussianModel.prune_points rebuilds the flat store (and the Adam moments of a model in
    training).  Returns the number of surfels removed."""
    if not torch.is_tensor(mask) or mask.dtype != torch.bool or mask.numel() != model.P:
        raise ValueError("%s: mask must be a bool tensor of the model's %d surfels" % (WHO, model.P))
    mask = mask.reshape(-1).to(model.device)
    if model.xyz_gradient_accum.shape[0] != model.P:      # a loaded model that was never set up for training: no statistics to carry over
        model.xyz_gradient_accum = torch.zeros((model.P, 1), device=model.device)
        model.denom = torch.zeros((model.P, 1), device=model.device)
    if model.max_radii2D.shape[0] != model.P:
        model.max_radii2D = torch.zeros((model.P,), device=model.device)
    before = model.P
    model.prune_points(~mask)
    return before - model.P


def report(contrib, out=print):
    """Counts, and the histogram of max_w per decade"""
    mw = contrib.max_w.cpu().numpy().astype(np.float64)
    views = contrib.views.cpu().numpy()
    P = contrib.P
    out("%d surfels over %d views: %d unseen, %d never composited, %d dominate a pixel" %
        (P, contrib.next_tag - 1, int((views == 0).sum()), int((mw == 0).sum()), int((contrib.dominant.cpu().numpy() > 0).sum())))
    lo = 0.0
    for d in range(-7, 1):
        hi = 10.0 ** d
        n = int(((mw > lo) & (mw <= hi)).sum()) if d > -7 else int(((mw > 0) & (mw <= hi)).sum())
        out("  max_w in (%s, 1e%d]: %d (%.1f %%)" % ("0" if d == -7 else "1e%d" % (d - 1), d, n, 100.0 * n / max(P, 1)))
        lo = hi


# ------------------------------------------------------------------------------------------------ CLI
def build_parser():
    ap = argparse.ArgumentParser(description="Prune a trained model by what its surfels contribute to the training views (CONTRIB.md)")
    ap.add_argument("-m", "--model_path", type=str, required=True, help="the model directory (cameras.json, point_cloud/)")
    ap.add_argument("-s", "--source_path", type=str, default=None, help="the capture: its training cameras instead of cameras.json")
    ap.add_argument("--iteration", type=int, default=-1)
    ap.add_argument("--min_max_weight", type=float, default=None, help="keep the surfels whose largest blend weight reaches this")
    ap.add_argument("--min_views", type=int, default=None, help="keep the surfels seen (composited or ending a pixel) in at least this many views")
    ap.add_argument("--keep", type=int, default=None, help="keep at most this many surfels, the best by --score")
    ap.add_argument("--keep_ratio", type=float, default=None, help="keep at most this fraction of the surfels, the best by --score")
    ap.add_argument("--score", type=str, default="sum", choices=SCORES)
    ap.add_argument("--white_background", action="store_true")
    ap.add_argument("--report", action="store_true", help="print counts and the histogram of the largest weight per decade; write nothing")
    ap.add_argument("--out", type=str, default=None, help="the pruned .ply (default point_cloud/iteration_N/point_cloud_pruned.ply)")
    return ap


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.keep is not None and args.keep_ratio is not None:
        raise SystemExit("give --keep or --keep_ratio, not both")
    import surfel_mesh
    gaussians, cams, it, folder, pipe, bg = surfel_mesh.open_model(args, torch.device("cuda:0"))
    c = contribution(gaussians, cams, pipe, bg)
    if args.report:
        report(c)
        return 0
    mask = prune_mask(c, min_max_weight=args.min_max_weight, min_views=args.min_views, keep=args.keep, keep_ratio=args.keep_ratio, score=args.score)
    c.save(os.path.join(folder, "contribution.npz"))
    removed = prune_model(gaussians, mask)
    out = args.out or os.path.join(folder, "point_cloud_pruned.ply")
    gaussians.save_ply(out)
    print("%d of %d surfels removed over %d views -> %s" % (removed, c.P, len(cams), out))
    return 0


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    sys.exit(main())
