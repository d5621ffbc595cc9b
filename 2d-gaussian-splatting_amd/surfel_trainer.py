"""Training driver on MI355X: the loop of /root/reference/train.py:31-144 on the fused kernels, with the
view-parallel multi-GPU step of surfel_dist.py.

Per iteration (1 view per GPU):  rasterize -> photometric loss (1 fwd + 1 bwd kernel) -> regularisers straight from allmap
(1 fwd + 1 bwd kernel) -> rasterizer backward writing into the flat gradient store -> densification statistics (1 kernel)
-> [RCCL: one all-reduce of the 40 B/surfel geometry gradients + one all-gather of 12 B/surfel/rank colour gradients, from which
the 192 B/surfel SH gradients are rebuilt locally] -> fused Adam + activations (2 kernels).  The reference spends ~150 small PyTorch
kernels on the same work around its rasterizer.

Semantics kept from the reference: learning-rate schedule, SH degree every 1000 iterations, lambda_dist after 3000 and
lambda_normal after 7000 iterations, densify/prune/opacity-reset schedule, no optimiser update on the iterations that
re-create the parameters (densification), Adam(eps=1e-15).  Multi-GPU: G views per step with averaged gradients; the
densification statistics are accumulated locally and all-reduced only when a densification is due.
"""
import math
import random
import time
from types import SimpleNamespace

import numpy as np
import torch
import torch.distributed as dist

import surfel_dist
import surfel_native as _n
from surfel_losses import scalars_from_band_sums, train_loss, train_loss_band, train_loss_manual, train_loss_manual_backward
from surfel_model import COLOUR_FLOATS, GEOM_FLOATS, GaussianModel, exchange_collectives, exchange_same_view
from surfel_render import Camera, post_consts_rows, rasterize, rasterize_manual, rasterize_manual_backward, render


def optimization_params(**over):
    """Defaults of arguments/__init__.py:75-95 (OptimizationParams)."""
    d = dict(iterations=30_000, position_lr_init=0.00016, position_lr_final=0.0000016, position_lr_delay_mult=0.01,
             position_lr_max_steps=30_000, feature_lr=0.0025, opacity_lr=0.05, scaling_lr=0.005, rotation_lr=0.001,
             percent_dense=0.01, lambda_dssim=0.2, lambda_dist=0.0, lambda_normal=0.05, opacity_cull=0.05,
             densification_interval=100, opacity_reset_interval=3000, densify_from_iter=500, densify_until_iter=15_000,
             densify_grad_threshold=0.0002, dist_from_iter=3000, normal_from_iter=7000,
             sh_degree_interval=1000)          # train.py:61-62 hard-codes the 1000
    d.update(over)
    return SimpleNamespace(**d)


def scale_schedule(opt, n, lr="linear"):
    """View-parallel training sees n views per step.  This returns the schedule with every iteration count divided by n (total
    iterations, position-lr horizon, densification window / interval, opacity reset, regulariser and SH-degree onsets), so that
    the run consumes the SAME number of images as the reference's 1-view-per-step schedule and every event happens after the same
    number of images, and with the learning rates scaled: lr = "linear" (x n, default), "sqrt" (x sqrt n) or "none".
    PSNR-parity experiment (profiles/r02_psnr_parity.md, N = 2 / 4 / 8): "linear" keeps the train PSNR of the 1-view reference
    run (+0.05 ... +1.0 dB) in 1/n of the steps; "none" loses 3 - 4 dB at N >= 4; keeping the step count instead (no call to this
    function, gradients averaged) is never below the reference (+1.9 ... +3.4 dB: it sees n x the images)."""
    n = max(1, int(n))
    d = dict(vars(opt))
    f = {"linear": float(n), "sqrt": float(n) ** 0.5, "none": 1.0}[lr]
    for k in ("position_lr_init", "position_lr_final", "feature_lr", "opacity_lr", "scaling_lr", "rotation_lr"):
        d[k] = d[k] * f
    for k in ("iterations", "position_lr_max_steps", "densification_interval", "opacity_reset_interval", "densify_from_iter",
              "densify_until_iter", "dist_from_iter", "normal_from_iter", "sh_degree_interval"):
        d[k] = max(1, int(round(d[k] / n)))
    return SimpleNamespace(**d)


def pipeline_params(**over):
    """Defaults of arguments/__init__.py:66-72 (PipelineParams)."""
    d = dict(convert_SHs_python=False, compute_cov3D_python=False, depth_ratio=0.0, debug=False)
    d.update(over)
    return SimpleNamespace(**d)


def psnr(img1, img2):
    """utils/image_utils.py:19-21."""
    mse = ((img1 - img2) ** 2).reshape(img1.shape[0], -1).mean(1, keepdim=True)
    return 20 * torch.log10(1.0 / torch.sqrt(mse))


# ------------------------------------------------------------------------------------------------ synthetic captures
def look_at(eye, target=(0.0, 0.0, 0.0), up=(0.0, -1.0, 0.0)):
    """(R, T) in the reference's Camera convention: R = C2W rotation (columns = camera x right, y down, z forward), T = W2C translation."""
    eye = np.asarray(eye, np.float64); target = np.asarray(target, np.float64)
    fwd = target - eye; fwd /= np.linalg.norm(fwd)
    right = np.cross(fwd, np.asarray(up, np.float64)); right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd], axis=1)
    return R, -R.T @ eye


def orbit_cameras(n_views, W, H, radius=4.0, fov_deg=50.0, device="cuda", seed=0):
    """Cameras on a sphere of `radius` looking at the origin (NeRF-synthetic style), images filled in later."""
    rng = np.random.default_rng(seed)
    fovx = math.radians(fov_deg)
    fovy = 2 * math.atan(math.tan(fovx / 2) * H / W)
    cams = []
    for i in range(n_views):
        az = 2 * math.pi * (i + 0.5 * rng.uniform()) / n_views
        el = math.radians(rng.uniform(-25, 35))
        eye = radius * np.array([math.cos(el) * math.cos(az), -math.sin(el), math.cos(el) * math.sin(az)])
        R, T = look_at(eye)
        cams.append(Camera(colmap_id=i, R=R, T=T, FoVx=fovx, FoVy=fovy, image=torch.zeros(3, H, W), image_name="syn_%03d" % i, uid=i,
                           data_device=device))
    return cams


def cameras_extent(cams):
    """Scene radius as scene/dataset_readers.py:40-64 (getNerfppNorm) computes it: 1.1 x max distance of a camera from the mean."""
    c = torch.stack([cam.camera_center for cam in cams]).double().cpu().numpy()
    return float(np.linalg.norm(c - c.mean(0, keepdims=True), axis=1).max() * 1.1)


def synthetic_object(P, device, seed=0, extent=1.2, px_scale=0.03):
    """A ground-truth surfel set: a thick random shell of oriented discs around the origin (raw, pre-activation parameters)."""
    g = torch.Generator().manual_seed(seed)
    d = torch.randn((P, 3), generator=g); d = d / d.norm(dim=1, keepdim=True)
    r = extent * (0.6 + 0.4 * torch.rand((P, 1), generator=g))
    xyz = d * r
    # discs roughly tangent to the shell: rotate z-axis onto the radial direction
    z = torch.tensor([0.0, 0.0, 1.0]).expand(P, 3)
    axis = torch.cross(z, d, dim=1); s = axis.norm(dim=1, keepdim=True).clamp_min(1e-8); axis = axis / s
    ang = torch.atan2(s.squeeze(1), (z * d).sum(1))
    quat = torch.cat([torch.cos(ang / 2)[:, None], axis * torch.sin(ang / 2)[:, None]], dim=1)
    scaling = torch.log(px_scale * torch.exp(0.4 * torch.randn((P, 2), generator=g)))
    opacity = torch.logit(torch.rand((P, 1), generator=g) * 0.5 + 0.45)
    f_dc = torch.randn((P, 1, 3), generator=g) * 0.8
    f_rest = torch.randn((P, 15, 3), generator=g) * 0.05
    m = GaussianModel(3, device=device)
    m.set_parameters(xyz, f_dc, f_rest, opacity, scaling, quat)
    m.active_sh_degree = 3
    return m


def capture_views(gt_model, cams, background, pipe=None):
    """Fill the cameras' original_image with renders of the ground-truth surfels (the synthetic stand-in for a dataset)."""
    pipe = pipe or pipeline_params()
    with torch.no_grad():
        for cam in cams:
            img = render(cam, gt_model, pipe, background)["render"]
            cam.original_image = img.clamp(0.0, 1.0).contiguous()
    return cams


# ------------------------------------------------------------------------------------------------ the loop
class Trainer:
    def __init__(self, model, cams, opt=None, pipe=None, white_background=False, extent=None, seed=0, sharding="views", first_iter=0,
                 rehearse_exchange=False, solo=False, logger=None, prune_at=(), prune_min_max_weight=None, prune_min_views=None):
        """sharding (N > 1): "views" = every rank trains on its own view per step (default, BASELINE config 4); "bands" = all ranks
        render row bands of the SAME view (tile-band sharding, BASELINE config 5): every rank evaluates the loss on ITS band plus a
        32-row halo received from its two neighbours (surfel_losses.train_loss_band), back-propagates its own rows, and the
        per-surfel gradients of the bands ADD UP to the single-GPU gradient — ONE all-reduce of 52 B/surfel (geometry + colour
        gradients; the camera is shared, so the SH gradients are rebuilt from the SUM of the colour gradients), no averaging.
        Band edges follow the previous frames' instances per tile row (re-balanced every `rebalance_every` iterations).
        rehearse_exchange: take the view-parallel step (schedule, collectives, split optimiser) even with a single rank — the
        N > 1 code path run against the real backend on one GPU (tests/test_gpu_train.py, scripts/rccl_selfcheck.py).
        solo: ignore an initialised process group — this rank trains alone (bench.py: every rank prepares the same trained state by
        itself, deterministically, before the timed view-parallel Trainer synchronises the replicas).
        logger: a surfel_log.EventWriter (LOG.md): rank 0 appends every step's scalars to it with one launch behind the step's work; None
        (the default): no launch, no buffer, no thread.
        prune_at: iterations after which the model is pruned by blend contribution (CONTRIB.md, "prune and recover"): a contribution pass
        over the training cameras, then the surfels whose largest blend weight stays below prune_min_max_weight or that fewer than
        prune_min_views views saw are removed, behind the iteration's own densification if it has one.  Empty (the default): no launch,
        no allocation, the same training bits.  One GPU only."""
        if sharding not in ("views", "bands"):
            raise ValueError("sharding must be 'views' or 'bands'")
        self.sharding = sharding
        self.model, self.cams = model, cams
        self.opt = opt or optimization_params()
        self.pipe = pipe or pipeline_params()
        self.white_background = white_background
        self.background = torch.tensor([1.0, 1.0, 1.0] if white_background else [0.0, 0.0, 0.0], dtype=torch.float32, device=model.device)
        self.extent = extent if extent is not None else cameras_extent(cams)
        self.world = dist.get_world_size() if (not solo and dist.is_available() and dist.is_initialized()) else 1
        self.rank = dist.get_rank() if self.world > 1 else 0
        self.seed = seed
        self._rng = random.Random(seed)
        self._stack = []
        self.iteration = int(first_iter)      # resume: the checkpoint's iteration (train.py:37-39), so that the lr / SH / densify schedules continue
        self.last = {}
        self.logger = logger
        self.prune_at = frozenset(int(i) for i in (prune_at or ()))
        self.prune_rules = dict(min_max_weight=prune_min_max_weight, min_views=prune_min_views)
        self.pruned = []                # [(iteration, surfels before, surfels after)]
        if self.prune_at and prune_min_max_weight is None and prune_min_views is None:
            raise ValueError("prune_at needs prune_min_max_weight or prune_min_views")
        self._lambdas = (0.0, 0.0)
        self._epoch, self._epoch_views, self._epoch_campos, self._centers = -1, None, None, None
        self._one = torch.ones((), dtype=torch.float32, device=model.device)
        # test handles (tests/test_gpu_train.py compares each with its bit-identical alternative)
        self.lazy_count = True          # forward without the host wait for the instance count (_forward_backward)
        self.lazy_overflows = 0
        self.manual_chain = True        # forward / backward of the iteration driven without autograd (_forward_backward)
        self.fused_update = True        # statistics + Adam in one launch (surfel_train_update) where nothing comes between them
        self.views_per_step = 1         # single process: > 1 = accumulate that many views per optimiser step (_step_accumulate)
        self.rebalance_every = 8        # bands: iterations between re-balancing the band edges (one small all-gather + D2H)
        self._row_weights = None        # bands: running mean of tile instances per 16-row tile row (host list) of frames of ...
        self._row_weights_hw = None     # ... this (height, width): cameras of another resolution start a fresh mean
        self.wire = {"total": 0}        # bytes on the wire per GPU of the most recent step, by collective (surfel_dist.wire_bytes_per_step)
        self.time_exchange = False      # bench: bracket the stream waits on the exchange with events -> self.exchange_events
        self.exchange_events = []
        # RCCL: asynchronous collectives with stream-level waits (SH-block Adam overlaps the geometry all-reduce); other backends
        # (gloo rehearsals stage through the host and block) take the plain synchronous form
        self._exchange = self.world > 1 or (bool(rehearse_exchange) and dist.is_available() and dist.is_initialized())
        self._async_exchange = self._exchange and dist.get_backend() == "nccl"
        # views + RCCL: the all-gather of the colour gradients starts inside the rasterizer's backward, as soon as the kernel that
        # finalises them is on the stream (surfel_set_backward_hook), and overlaps the per-surfel geometry chain rule.  The split
        # costs a second pass over the gradient records (measured +15 us at C2, +208 us at C4: scripts/hook_cost.py) and buys up to
        # min(gather time, chain-rule time): worth it once the gather is long, i.e. from 4 ranks on (12 B/surfel/rank received)
        # ... or not: RCCL's launch latency, the link count and the frame size decide, so with more than one rank it is MEASURED at
        # start-up ("auto": four iterations with the early gather, four without, device time by events on the compute stream, the
        # slower rank decides for all: _probe_early_gather) — results are bit-identical either way.
        self.early_gather = True if rehearse_exchange else ("auto" if (self.world > 1 and self._async_exchange and sharding == "views") else False)
        self.early_gather_probe = None      # {"early_ms": .., "late_ms": .., "choice": ..} once decided
        self._eg_events, self._eg_first, self._eg_failed = [], None, False
        self._early, self._early_err = None, None
        if model.grad is None:
            model.training_setup(self.opt)
        if self.world > 1:
            if self.prune_at:
                raise ValueError("prune_at is a single-GPU option")
            self._sync_replicas()

    def _sync_replicas(self):
        """N > 1: every rank must start from the same model.  Surfel count and optimiser step are checked (a mismatch would make
        the fixed-size collectives hang or corrupt memory), then parameters, Adam moments and densification statistics are
        broadcast from rank 0 (create_from_pcd draws its rotations from the global RNG, so differently seeded ranks differ)."""
        m = self.model
        chk = torch.tensor([m.P, m.step_count, self.iteration], dtype=torch.int64, device=m.device)
        lo, hi = chk.clone(), chk.clone()
        dist.all_reduce(lo, op=dist.ReduceOp.MIN); dist.all_reduce(hi, op=dist.ReduceOp.MAX)
        if not torch.equal(lo, hi):
            raise RuntimeError("view-parallel ranks disagree on (surfels, optimiser step, iteration): min %s max %s" % (lo.tolist(), hi.tolist()))
        for t in (m.theta, m.m, m.v, m.xyz_gradient_accum, m.denom, m.max_radii2D):
            if t is not None and t.numel():
                dist.broadcast(t, src=0)
        m.refresh_activations()

    def _step_views(self):
        """(camera indices of ALL ranks for the current iteration, their camera centres [world,3] on the device).  Every rank
        computes the same schedule (surfel_dist.view_indices); it is built once per epoch, so a step costs no host RNG work
        and no device gather."""
        per_epoch = max(1, len(self.cams) // self.world)
        epoch, k = divmod(self.iteration - 1, per_epoch)
        if self._epoch != epoch:
            self._epoch = epoch
            self._epoch_views = surfel_dist.epoch_schedule(len(self.cams), self.world, epoch, self.seed)
            if self._centers is None:
                self._centers = torch.stack([c.camera_center for c in self.cams]).contiguous()
            idx = torch.tensor(self._epoch_views, dtype=torch.long, device=self._centers.device)
            self._epoch_campos = self._centers[idx.reshape(-1)].reshape(per_epoch, self.world, 3).contiguous()
        return self._epoch_views[k], self._epoch_campos[k]

    def _next_camera(self):
        if self._exchange and self.sharding == "views":
            return self.cams[self._step_views()[0][self.rank]]
        if not self._stack:                       # train.py:64-67: pop a random view from a refilled stack
            self._stack = list(range(len(self.cams)))
        return self.cams[self._stack.pop(self._rng.randint(0, len(self._stack) - 1))]

    def _reduce_stats(self):
        m = self.model
        packed = torch.cat([m.xyz_gradient_accum, m.denom], dim=1).contiguous()
        dist.all_reduce(packed, op=dist.ReduceOp.SUM)
        m.xyz_gradient_accum, m.denom = packed[:, :1].contiguous(), packed[:, 1:2].contiguous()
        dist.all_reduce(m.max_radii2D, op=dist.ReduceOp.MAX)

    def step(self):
        """One training iteration (train.py:54-138).  Returns nothing; `self.last` holds device scalars for logging."""
        if self.world == 1 and self.views_per_step > 1:
            self._step_accumulate(self.views_per_step)
        else:
            it, lam_n, lam_d = self._begin_step()
            cam = self._next_camera()
            self.model.bind(sh_grad=False)      # the SH gradients are rebuilt inside the optimiser kernel from the colour gradients
            if self.world > 1 and self.sharding == "bands":
                self._step_band(it, cam, lam_n, lam_d)
            else:
                self._step_view(it, cam, lam_n, lam_d)
        if self.prune_at and self.iteration in self.prune_at:
            self._prune_by_contribution()
        if self.logger is not None and self.rank == 0:
            # the step's work is queued: the deferred loss scalars are valid on the stream, and `points` is the count the step rendered
            # (training_report runs before the densification, train.py:119-132)
            self.logger.append(self.iteration, self.last["points"], self.last["scalars"], *self._lambdas)

    def _prune_by_contribution(self):
        """prune_at: behind the iteration (and its densification, if it had one) — never inside it."""
        import surfel_prune
        m = self.model
        with torch.no_grad():
            c = surfel_prune.contribution(m, self.cams, self.pipe, self.background)
            before = m.P
            surfel_prune.prune_model(m, surfel_prune.prune_mask(c, **self.prune_rules))
        self.pruned.append((self.iteration, before, m.P))

    def _begin_step(self):
        """Advance the iteration, set its learning rate and SH degree; returns (iteration, lambda_normal, lambda_dist)."""
        self.iteration += 1
        it, opt = self.iteration, self.opt
        self.model.update_learning_rate(it)
        if it % getattr(opt, "sh_degree_interval", 1000) == 0:
            self.model.oneupSHdegree()
        self._lambdas = ((opt.lambda_normal if it > opt.normal_from_iter else 0.0), (opt.lambda_dist if it > opt.dist_from_iter else 0.0))
        return (it,) + self._lambdas

    def _step_view(self, it, cam, lam_n, lam_d):
        """One GPU, or view-parallel (N ranks, or the world-1 rehearsal): every rank trains on its own view."""
        opt, m = self.opt, self.model
        stats_live = it < opt.densify_until_iter
        self.wire = surfel_dist.wire_bytes_per_step(m.P, self.world, self.sharding, stats_live)
        early = self._probe_early_gather() and self._async_exchange and it < opt.iterations
        radii, scalars, g2d = self._forward_backward(cam, lam_n, lam_d, early)
        self.last = dict(loss=scalars[5], scalars=scalars, points=m.P, radii=radii)     # [Ll1, ssim, normal_err, dist, photometric, total] on the device
        with torch.no_grad():
            if self.fused_update and not self._exchange and it < opt.iterations and not self._is_event_iteration(it):
                # statistics + optimiser step as ONE launch where nothing can come between them (single GPU, no densification /
                # opacity reset this iteration): two launch boundaries and the statistics' latency-bound kernel fewer
                m.update_step((cam.camera_center[None], m.gcol[None]), stats=(g2d, radii) if stats_live else None)
                return
            rebuilt = False
            if stats_live:
                m.add_densification_stats(g2d, radii=radii)
                rebuilt = self._schedule_events(it)
            if it < opt.iterations and not rebuilt:     # re-created parameters carry no gradient in the reference: no update
                if self._exchange:
                    self._exchange_step()
                else:
                    m.optimizer_step(grad_scale=1.0, colour_grads=(cam.camera_center[None], m.gcol[None]))
            if self._early is not None:      # an iteration without an optimiser step (parameters re-created): retire the gather
                self._early[1].wait()
                self._early = None

    def _forward_backward(self, cam, lam_n, lam_d, early):
        """Render, loss and backward of one view; returns (radii, loss scalars, dL/dmeans2D).
        Lazily counted forward (include/surfel_hip.h: SURFEL_OPT_LAZY_COUNT): the host does not wait for the frame's instance count in
        the middle of the iteration — it enqueues loss and backward behind the forward and collects the count afterwards, when it has
        long arrived; a frame that overflowed its binning capacity (rare) is rendered again with exact sizes, loss and backward with
        it, before anything irreversible (statistics, optimiser step, collectives) has happened.
        The chain (rasterizer -> loss -> loss backward -> rasterizer backward) is fixed: driven by hand (surfel_native.ManualCtx) it
        costs a fraction of the host time autograd spends on it — engine, worker-thread hand-over, five parameter gates — with the same
        kernels and bits; compute_cov3D_python trains through PyTorch code and needs autograd.
        early: the colour all-gather starts inside the rasterizer's backward (_on_colour_ready)."""
        opt, m, pipe = self.opt, self.model, self.pipe
        reg = lam_n > 0.0 or lam_d > 0.0
        lazy = self.lazy_count and not early
        manual = self.manual_chain and not getattr(pipe, "compute_cov3D_python", False)
        for bits in ((_n.OPT_LAZY_COUNT, _n.OPT_EXACT_BINNING) if lazy else (0,)):
            loss_args = (pipe.depth_ratio, opt.lambda_dssim, lam_n, lam_d)
            if manual:
                with torch.no_grad():
                    rctx, image, radii, allmap = rasterize_manual(cam, m, pipe, self.background, debug_bits=bits)
                    lctx, loss, scalars = train_loss_manual(image, allmap if reg else None, cam.original_image, cam.post_consts() if reg else None,
                                                            *loss_args, defer_scalars=True)
            else:
                image, radii, allmap, means2D = rasterize(cam, m, pipe, self.background, zero_means2D=False, debug_bits=bits)
                loss, scalars = train_loss(image, allmap if reg else None, cam.original_image, cam.post_consts() if reg else None,
                                           *loss_args, defer_scalars=True)      # (read after the backward below)
            if early:
                self._early, self._early_err = None, None
                _n.set_backward_hook(self._on_colour_ready)
            try:
                if manual:
                    with torch.no_grad():
                        g2d = rasterize_manual_backward(rctx, *train_loss_manual_backward(lctx, self._one))
                else:
                    torch.autograd.backward(loss, grad_tensors=self._one)        # cached seed gradient: no ones_like fill per iteration
                    g2d = means2D.grad
            finally:
                if early:
                    _n.set_backward_hook(None)
            if not lazy:
                break
            try:
                import diff_surfel_rasterization as dsr
                dsr.finish_count()
                break
            except _n.CapacityOverflow:
                self.lazy_overflows += 1
                lazy = False      # second pass: exact binning, count known when the forward returns
        if self._early_err is not None:
            # the early all-gather could not be launched from inside the backward: dL/dcolour is final regardless (the split
            # kernel ran), so the step continues with the gather-after-backward form and the early form stays off
            import warnings
            warnings.warn("early colour all-gather disabled after: %r" % (self._early_err,))
            if self.early_gather == "auto":
                # mid-probe: the other ranks still expect this rank in the verdict's all-reduce (_probe_early_gather) — keep the state
                # machine running, take the late form from here on, and vote "early = never" when the verdict is due
                self._eg_failed = True
            else:
                self.early_gather = False
            self._early, self._early_err = None, None
        return radii, scalars, g2d

    def _exchange_step(self):
        """View-parallel optimiser step: all-reduce of the 40 B/surfel geometry prefix + all-gather of 12 B/surfel/rank colour
        gradients; the 192 B/surfel SH gradients are rebuilt from them (exact, rank-ordered sum) instead of being all-reduced."""
        m = self.model
        campos_all = self._step_views()[1]
        scale = 1.0 / self.world      # views: average
        if not self._async_exchange:
            gcol_all = exchange_collectives(m.grad, m.gcol, m.P)
            m.optimizer_step(grad_scale=scale, colour_grads=(campos_all, gcol_all))
            return
        if self._early is not None:      # the gather has been in flight since the middle of the backward
            gcol_all, w_gather = self._early
            self._early = None
            w_reduce = dist.all_reduce(m.grad[:GEOM_FLOATS * m.P], op=dist.ReduceOp.SUM, async_op=True)
        else:
            gcol_all, w_gather, w_reduce = exchange_collectives(m.grad, m.gcol, m.P, async_op=True)
        self._timed_wait(w_gather)   # stream-level wait: the SH block updates while the geometry all-reduce is in flight
        m.optimizer_step(grad_scale=scale, colour_grads=(campos_all, gcol_all), parts=1)
        self._timed_wait(w_reduce)
        m.optimizer_step(grad_scale=scale, colour_grads=(campos_all, gcol_all), parts=2)

    def _step_band(self, it, cam, lam_n, lam_d):
        """Tile-band sharding (N > 1): every rank renders its row band of the SAME view (see __init__)."""
        opt, m = self.opt, self.model
        reg = lam_n > 0.0 or lam_d > 0.0
        stats_live = it < opt.densify_until_iter
        H, W = int(cam.image_height), int(cam.image_width)
        if self._row_weights_hw != (H, W):      # real capture sets mix resolutions: the running weights belong to one of them
            self._row_weights, self._row_weights_hw = None, (H, W)
        bounds = surfel_dist.band_bounds(H, self.world, self._row_weights, multiple=surfel_dist.HALO)
        y0, y1 = bounds[self.rank]
        # the densification statistic of the view = norm of the SUM over bands: it rides in the same all-reduce, right
        # behind the colour block (both live in the SH section of the gradient store, unused in fused-SH mode)
        arena2d = m.grad[(GEOM_FLOATS + COLOUR_FLOATS) * m.P:(GEOM_FLOATS + COLOUR_FLOATS + 3) * m.P].view(m.P, 3)
        import diff_surfel_rasterization as dsr
        dsr._grad_arena["means2D"] = arena2d
        image_b, radii, allmap_b, _ = rasterize(cam, m, self.pipe, self.background, zero_means2D=False, band=(y0, y1))
        ext = surfel_dist.exchange_halo(torch.cat([image_b, allmap_b], 0) if reg else image_b, bounds, H)
        top, bot = surfel_dist.halo_rows(bounds, self.rank, H)
        gt_ext = cam.original_image[:, y0 - top:y1 + bot]
        consts = post_consts_rows(cam.post_consts(), y0 - top) if reg else None
        loss, sums = train_loss_band(ext[:3], ext[3:] if reg else None, gt_ext, consts, self.pipe.depth_ratio, opt.lambda_dssim, lam_n, lam_d,
                                     (top, top + (y1 - y0)), (H, W))
        sums = sums.clone()
        dist.all_reduce(sums, op=dist.ReduceOp.SUM)           # 16 bytes: the full-image loss terms, for logging
        scalars = scalars_from_band_sums(sums, float(3 * H * W), float(H * W), opt.lambda_dssim, lam_n, lam_d)
        self.wire = surfel_dist.wire_bytes_per_step(m.P, self.world, self.sharding, stats_live,
                                                    surfel_dist.halo_bytes(bounds, self.rank, H, W, 10 if reg else 3))
        torch.autograd.backward(loss, grad_tensors=self._one)
        self.last = dict(loss=scalars[5], scalars=scalars, points=m.P, radii=radii)
        with torch.no_grad():
            # ONE all-reduce: geometry 10 | colour 3 (| means2D statistic 3) floats per surfel
            n_f = GEOM_FLOATS + COLOUR_FLOATS + (3 if stats_live else 0)
            w_same = dist.all_reduce(m.grad[:n_f * m.P], op=dist.ReduceOp.SUM, async_op=self._async_exchange)
            if stats_live:
                radii = radii.clone(); dist.all_reduce(radii, op=dist.ReduceOp.MAX)      # visibility = union of the bands
            if self._async_exchange:
                self._timed_wait(w_same)
            self._rebalance_bands(cam)
            rebuilt = False
            if stats_live:
                m.add_densification_stats(arena2d, radii=radii)
                rebuilt = self._schedule_events(it, bands=True)
            if it < opt.iterations and not rebuilt:
                # partial gradients of one view add up (no averaging); the SH block is rebuilt from the summed colour gradients
                m.optimizer_step(grad_scale=1.0, colour_grads=(cam.camera_center[None], m.gcol[None]))

    EG_WARM, EG_LEN = 2, 4      # start-up probe: iterations skipped, iterations per setting

    @staticmethod
    def decide_early_gather(early_ms, late_ms):
        """The early gather pays a second pass over the gradient records: keep it only when it wins by more than measurement noise."""
        return early_ms < 0.98 * late_ms

    def _probe_early_gather(self):
        """early_gather == "auto": whether THIS iteration takes the early gather; after 2 x EG_LEN probe iterations the faster setting
        (max over ranks of the device time) is fixed for the rest of the run."""
        if self.early_gather != "auto":
            return bool(self.early_gather)
        if self._eg_first is None:
            # the two windows must time the same kind of iteration: start behind the warm-up at the first iteration from which
            # 2 x EG_LEN iterations hold no densification / opacity reset (a function of the iteration number: the same on every rank)
            first = self.iteration + self.EG_WARM
            while any(self._is_event_iteration(first + k) for k in range(2 * self.EG_LEN + 1)):
                first += 1
            self._eg_first = first
        ph = self.iteration - self._eg_first
        if ph < 0:
            return False
        if ph in (0, self.EG_LEN, 2 * self.EG_LEN):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            self._eg_events.append(ev)
        if ph < self.EG_LEN:
            return not self._eg_failed      # (a rank whose early gather failed takes the late form: the same collectives, later)
        if ph < 2 * self.EG_LEN:
            return False
        try:
            e0, e1, e2 = self._eg_events
            e2.synchronize()
            t = torch.tensor([e0.elapsed_time(e1), e1.elapsed_time(e2)], dtype=torch.float32, device=self.model.device)
        except Exception:      # noqa: BLE001 — no timing, no early gather; every rank still joins the collective below
            t = torch.tensor([1.0, 0.0], dtype=torch.float32, device=self.model.device)
        if self._eg_failed:      # this rank cannot launch the early gather: MAX over the ranks turns every rank's verdict to "late"
            t = torch.tensor([3.0e38, 0.0], dtype=torch.float32, device=self.model.device)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        early_ms, late_ms = (float(x) / self.EG_LEN for x in t.tolist())
        self.early_gather = self.decide_early_gather(early_ms, late_ms)
        self.early_gather_probe = {"early_ms_per_step": round(early_ms, 4), "late_ms_per_step": round(late_ms, 4), "choice": "early" if self.early_gather else "late"}
        self._eg_events = []
        return self.early_gather

    def _is_event_iteration(self, it):
        """Does iteration `it` densify / prune or reset the opacities (_schedule_events)?  Those iterations cost more and skip the optimiser step."""
        opt = self.opt
        if it < opt.densify_until_iter and it > opt.densify_from_iter and it % opt.densification_interval == 0:
            return True
        return it < opt.densify_until_iter and (it % opt.opacity_reset_interval == 0 or (self.white_background and it == opt.densify_from_iter))

    def _on_colour_ready(self):
        """Called by the C library inside the rasterizer's backward (autograd's thread, the forward's stream) once dL/dcolour is
        final on the stream: launch the all-gather of this rank's colour gradients now.  Exceptions cannot cross the C frame:
        they are parked and re-raised by step()."""
        try:
            m = self.model
            gall = torch.empty((dist.get_world_size(), m.P, 3), dtype=torch.float32, device=m.device)
            self._early = (gall, dist.all_gather_into_tensor(gall, m.gcol, async_op=True))
        except Exception as e:      # noqa: BLE001
            self._early, self._early_err = None, e

    def _schedule_events(self, it, bands=False):
        """Densification and opacity reset when due (train.py:129-135); returns whether the parameters were re-created."""
        opt, m = self.opt, self.model
        rebuilt = False
        if it > opt.densify_from_iter and it % opt.densification_interval == 0:
            if self.world > 1 and not bands:
                self._reduce_stats()
            size_threshold = 20 if it > opt.opacity_reset_interval else None
            gen = None
            if self.world > 1:       # identical split samples on every rank
                gen = torch.Generator(device=m.device); gen.manual_seed(self.seed * 1_000_003 + it)
            m.densify_and_prune(opt.densify_grad_threshold, opt.opacity_cull, self.extent, size_threshold, generator=gen)
            rebuilt = True
        if it % opt.opacity_reset_interval == 0 or (self.white_background and it == opt.densify_from_iter):
            m.reset_opacity()
            if not rebuilt:      # the reference re-creates only the opacity parameter: its update is skipped this iteration
                m._gv["opacity"].zero_()
        return rebuilt

    def _step_accumulate(self, n):
        """One optimiser step on the AVERAGED gradients of n views rendered one after the other on this GPU — the optimisation
        semantics of n view-parallel ranks (same view schedule: surfel_dist.epoch_schedule; per-view densification statistics;
        SH gradients rebuilt from the n views' colour gradients) without the processes.  Used by the PSNR-parity experiment."""
        it, lam_n, lam_d = self._begin_step()
        opt, m = self.opt, self.model
        per_epoch = max(1, len(self.cams) // n)
        epoch, k = divmod(it - 1, per_epoch)
        if self._epoch != epoch:
            self._epoch, self._epoch_views = epoch, surfel_dist.epoch_schedule(len(self.cams), n, epoch, self.seed)
        views = [self.cams[v] for v in self._epoch_views[k]]
        reg = lam_n > 0.0 or lam_d > 0.0
        geo = torch.zeros(GEOM_FLOATS * m.P, device=m.device)
        gcols = torch.empty((n, m.P, 3), device=m.device)
        for r, cam in enumerate(views):
            m.bind(sh_grad=False)
            image, radii, allmap, means2D = rasterize(cam, m, self.pipe, self.background, zero_means2D=False)
            loss, scalars = train_loss(image, allmap if reg else None, cam.original_image, cam.post_consts() if reg else None,
                                       self.pipe.depth_ratio, opt.lambda_dssim, lam_n, lam_d)
            torch.autograd.backward(loss, grad_tensors=self._one)
            with torch.no_grad():
                geo += m.grad[:GEOM_FLOATS * m.P]; gcols[r].copy_(m.gcol)
                if it < opt.densify_until_iter:
                    m.add_densification_stats(means2D.grad, radii=radii)
        self.last = dict(loss=scalars[5], scalars=scalars, points=m.P, radii=radii)
        with torch.no_grad():
            rebuilt = self._schedule_events(it) if it < opt.densify_until_iter else False
            if it < opt.iterations and not rebuilt:
                m.grad[:GEOM_FLOATS * m.P].copy_(geo)
                campos = torch.stack([c.camera_center for c in views]).contiguous()
                m.optimizer_step(grad_scale=1.0 / n, colour_grads=(campos, gcols))

    def _timed_wait(self, work):
        """Stream-level wait on an asynchronous collective; with time_exchange the wait is bracketed by events on the compute
        stream — the elapsed time is what the exchange was NOT hidden behind compute (resolved by the caller after the run)."""
        if self.time_exchange:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(); work.wait(); e1.record()
            self.exchange_events.append((e0, e1))
        else:
            work.wait()

    def _rebalance_bands(self, cam):
        """bands: every `rebalance_every` iterations gather the ranks' tile instances per tile row (a few hundred bytes) into a
        running mean that the next iterations' band_bounds use as weights."""
        if self.rebalance_every <= 0 or self.iteration % self.rebalance_every != 0:
            return
        import diff_surfel_rasterization as dsr
        rows16 = (int(cam.image_height) + 15) // 16
        mine = dsr.tile_row_instances()
        full = torch.zeros((rows16,), dtype=torch.int64, device=self.model.device)
        y0 = surfel_dist.band_bounds(int(cam.image_height), self.world, self._row_weights, multiple=surfel_dist.HALO)[self.rank][0]
        full[y0 // 16:y0 // 16 + mine.numel()] = mine
        dist.all_reduce(full, op=dist.ReduceOp.SUM)
        w = full.to(torch.float64).cpu().tolist()
        self._row_weights = w if self._row_weights is None else [0.5 * a + 0.5 * b for a, b in zip(self._row_weights, w)]

    def evaluate(self, cams=None):
        """Mean PSNR / L1 over views (training_report, train.py:201-232)."""
        cams = cams or self.cams
        with torch.no_grad():
            ps, l1 = [], []
            for cam in cams:
                img = torch.clamp(render(cam, self.model, self.pipe, self.background)["render"], 0.0, 1.0)
                gt = torch.clamp(cam.original_image, 0.0, 1.0)
                ps.append(psnr(img, gt).mean()); l1.append((img - gt).abs().mean())
            return float(torch.stack(ps).mean()), float(torch.stack(l1).mean())


def viewer_metrics(tr):
    """What the serve loop sends with every frame (train.py:157-160): the point count and the photometric loss — of the last
    iteration, read from the device only when a viewer asks, where the reference keeps a running mean with an .item() per step."""
    return lambda: {"#": int(tr.model.P), "loss": float(tr.last["scalars"][4]) if tr.last else 0.0}


def serve_viewer(viewer, tr, source_path=""):
    """train.py:146-168 after a step: let a connected remote viewer (surfel_view.Viewer) look at the model; a no-op without one."""
    viewer.serve(tr.model, tr.pipe, tr.background, source_path, viewer_metrics(tr), tr.iteration, tr.opt.iterations)


def training(model, cams, opt=None, pipe=None, iterations=None, white_background=False, log_every=0, seed=0, viewer=None):
    """Run the loop; returns the Trainer (model trained in place).  log_every > 0 prints loss / points / it/s.  viewer: a
    surfel_view.Viewer that is served after every step (VIEWER.md); None (the default) touches no socket."""
    opt = opt or optimization_params()
    if iterations is not None:
        opt.iterations = iterations
    tr = Trainer(model, cams, opt, pipe, white_background, seed=seed)
    t0 = time.perf_counter()
    for _ in range(opt.iterations):
        tr.step()
        if viewer is not None:
            serve_viewer(viewer, tr)
        if log_every and tr.iteration % log_every == 0 and tr.rank == 0:
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print("[it %d] loss %.5f points %d  %.1f it/s" % (tr.iteration, float(tr.last["loss"]), model.P, tr.iteration / dt), flush=True)
    return tr


# ------------------------------------------------------------------------------------------------ CLI (train.py:31-144, 146-160, 251-278)
_MODEL_ARGS = ("sh_degree", "source_path", "model_path", "images", "resolution", "white_background", "data_device", "eval")
_OPTIMIZATION_ARGS = ("iterations", "position_lr_init", "position_lr_final", "position_lr_delay_mult", "position_lr_max_steps", "feature_lr",
                      "opacity_lr", "scaling_lr", "rotation_lr", "percent_dense", "lambda_dssim", "lambda_dist", "lambda_normal", "opacity_cull",
                      "densification_interval", "opacity_reset_interval", "densify_from_iter", "densify_until_iter", "densify_grad_threshold")


def parse_args(argv=None):
    """The reference's flags with its defaults (arguments/__init__.py:47-95, train.py:258-265), without the viewer's --ip / --port and
    the log's --tensorboard: those are parse_viewer_args', which main() lets take its flags out of the command line first."""
    import argparse
    import os
    ap = argparse.ArgumentParser(description="Train a 2-D Gaussian surfel model on a COLMAP or Blender capture",
                                 epilog="The remote viewer (VIEWER.md): --port PORT serves it while training, on --ip IP (default 127.0.0.1); "
                                        "without --port no listener exists.  --tensorboard writes a TensorBoard event file into the "
                                        "model folder (LOG.md); without it nothing is logged.")
    g = ap.add_argument_group("Loading Parameters")
    g.add_argument("--source_path", "-s", default="", type=str)
    g.add_argument("--model_path", "-m", default="", type=str)
    g.add_argument("--images", "-i", default="images", type=str)
    g.add_argument("--resolution", "-r", default=-1, type=int)
    g.add_argument("--white_background", "-w", default=False, action="store_true")
    g.add_argument("--sh_degree", default=3, type=int)
    g.add_argument("--data_device", default="cuda", type=str)
    g.add_argument("--eval", default=False, action="store_true")
    g.add_argument("--undistort", default=False, action="store_true", help="undistort a COLMAP capture whose cameras are SIMPLE_RADIAL, RADIAL, OPENCV "
                   "or FULL_OPENCV while it is loaded (UNDISTORT.md): sparse/0 else distorted/sparse/0, the -i folder else input/")
    g = ap.add_argument_group("Optimization Parameters")
    defaults = vars(optimization_params())
    for name in _OPTIMIZATION_ARGS:
        g.add_argument("--" + name, default=defaults[name], type=type(defaults[name]))
    g = ap.add_argument_group("Pipeline Parameters")
    g.add_argument("--depth_ratio", default=0.0, type=float)
    ap.add_argument("--test_iterations", nargs="+", type=int, default=[7_000, 30_000])
    ap.add_argument("--save_iterations", nargs="+", type=int, default=[7_000, 30_000])
    ap.add_argument("--quiet", action="store_true")
    ap.add_argument("--checkpoint_iterations", nargs="+", type=int, default=[])
    ap.add_argument("--start_checkpoint", type=str, default=None)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--prune_at", nargs="+", type=int, default=[], help="prune the model by blend contribution after these iterations and train on "
                    "(CONTRIB.md); needs --prune_min_max_weight or --prune_min_views.  Default: never")
    ap.add_argument("--prune_min_max_weight", type=float, default=None, help="--prune_at keeps the surfels whose largest blend weight over the training "
                    "views reaches this")
    ap.add_argument("--prune_min_views", type=int, default=None, help="--prune_at keeps the surfels that at least this many training views saw")
    ap.add_argument("--workers", type=int, default=4, help="image decoding threads (at most 8)")
    ap.add_argument("--decode", default="host", choices=["host", "device"], help="who decodes the capture's JPEG files: Pillow on the host threads "
                    "(the default) or the decoder on the device (JPEGDEC.md); the same cameras")
    args = ap.parse_args(argv)
    args.save_iterations = list(args.save_iterations) + [args.iterations]
    args.source_path = os.path.abspath(args.source_path)
    return args


def optimization_from_args(args):
    return optimization_params(**{name: getattr(args, name) for name in _OPTIMIZATION_ARGS})


def write_cfg_args(args):
    """model_path/cfg_args = str(Namespace(...)) of the loading parameters (train.py:146-160), which the reference's render.py and
    metrics.py evaluate back (arguments/__init__.py:97-117).  undistort=True is added only for a run with --undistort, so that
    surfel_mesh.py -s reloads the same cameras; without the flag the file is what it always was."""
    import argparse
    import os
    os.makedirs(args.model_path, exist_ok=True)
    path = os.path.join(args.model_path, "cfg_args")
    with open(path, "w") as f:
        cfg = {k: getattr(args, k) for k in _MODEL_ARGS}
        if getattr(args, "undistort", False):
            cfg["undistort"] = True
        f.write(str(argparse.Namespace(**cfg)))
    return path


def parse_viewer_args(argv=None):
    """(viewer flags, the rest of the command line): --ip (default 127.0.0.1) and --port (default: none).  A departure from the
    reference, which always binds 127.0.0.1:6009: the listener exists only when --port is given, so two runs on one machine do not
    collide and a run without the flag behaves as it always did."""
    import argparse
    ap = argparse.ArgumentParser(add_help=False, allow_abbrev=False)
    ap.add_argument("--ip", type=str, default="127.0.0.1", help="address the remote viewer's listener binds (with --port)")
    ap.add_argument("--port", type=int, default=None, help="serve the SIBR remote viewer on this port while training (default: no listener)")
    ap.add_argument("--tensorboard", action="store_true", help="write the reference's TensorBoard log (scalars per step, image panels at the "
                    "test iterations) as an event file into the model folder (LOG.md; default: no log)")
    return ap.parse_known_args(argv)


def make_viewer(vargs):
    """The remote viewer's listener for --port, or None: without the flag no socket object is created."""
    if vargs.port is None:
        return None
    import surfel_view
    return surfel_view.Viewer(vargs.ip, vargs.port)


def make_logger(vargs, model_path):
    """The event writer for --tensorboard, or None: without the flag no file, thread or buffer is created."""
    if not getattr(vargs, "tensorboard", False):
        return None
    import surfel_log
    return surfel_log.EventWriter(model_path)


def main(argv=None):
    """python surfel_trainer.py -s <capture> -m <model folder> [...]: trains, saves point_cloud/iteration_N at the save iterations (the
    last iteration always among them), checkpoints as (capture(), iteration), and reports L1 / PSNR of the test split and of a train
    subset at the test iterations."""
    import os
    import uuid
    from surfel_scene import Scene
    vargs, rest = parse_viewer_args(argv)
    args = parse_args(rest)
    if not args.model_path:
        args.model_path = os.path.join("./output/", str(uuid.uuid4())[0:10])
    say = (lambda *a, **k: None) if args.quiet else print
    say("Optimizing " + args.model_path)
    random.seed(args.seed); np.random.seed(args.seed); torch.manual_seed(args.seed)
    write_cfg_args(args)
    opt, pipe = optimization_from_args(args), pipeline_params(depth_ratio=args.depth_ratio)
    scene = Scene(args.source_path, args.model_path, images=args.images, resolution=args.resolution, white_background=args.white_background,
                  eval=args.eval, data_device=args.data_device, seed=args.seed, workers=args.workers, sh_degree=args.sh_degree, decode=args.decode,
                  undistort=args.undistort)
    model, first_iter = scene.gaussians, 0
    model.training_setup(opt)
    if args.start_checkpoint:
        model_params, first_iter = torch.load(args.start_checkpoint, weights_only=False)
        model.restore(model_params, opt)
    logger = make_logger(vargs, args.model_path)
    tr = Trainer(model, scene.getTrainCameras(), opt, pipe, args.white_background, extent=scene.cameras_extent, seed=args.seed, first_iter=first_iter,
                 logger=logger, prune_at=args.prune_at, prune_min_max_weight=args.prune_min_max_weight, prune_min_views=args.prune_min_views)
    train_cams = scene.getTrainCameras()
    reports = (("test", scene.getTestCameras()), ("train", [train_cams[i % len(train_cams)] for i in range(5, 30, 5)]))
    viewer = make_viewer(vargs)
    t0 = time.perf_counter()
    if logger is not None:
        logger.mark()      # iter_time of the first block counts from here, not from the writer's creation
    while tr.iteration < opt.iterations:
        tr.step()
        it = tr.iteration
        if viewer is not None:
            serve_viewer(viewer, tr, args.source_path)
        if it in args.test_iterations:
            for name, cams in reports:
                if cams:
                    if logger is not None:      # the same evaluation, with its numbers and the views' panels logged (LOG.md)
                        import surfel_log
                        ps, l1 = surfel_log.report(tr, logger, name, cams, first=it == args.test_iterations[0])
                    else:
                        ps, l1 = tr.evaluate(cams)
                    say("\n[ITER {}] Evaluating {}: L1 {} PSNR {}".format(it, name, l1, ps))
        if it in args.save_iterations:
            say("\n[ITER {}] Saving Gaussians".format(it))
            scene.save(it)
        if it in args.checkpoint_iterations:
            say("\n[ITER {}] Saving Checkpoint".format(it))
            torch.save((model.capture(), it), os.path.join(args.model_path, "chkpnt" + str(it) + ".pth"))
    if viewer is not None:
        viewer.close()
    if logger is not None:
        logger.close()
    torch.cuda.synchronize()
    say("\nTraining complete: %d iterations, %d points, %.1f s." % (tr.iteration - first_iter, model.P, time.perf_counter() - t0))
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
