"""Shared helpers for the parity tests: call the HIP path through the C ABI, call the oracle."""
import ctypes as C

import numpy as np


def scene_args(sc):
    """dict of numpy inputs in the reference's argument vocabulary from a synthetic / golden scene."""
    return dict(bg=sc["bg"], means3D=sc["means3D"], opacities=sc["opacities"], scales=sc["scales"],
                rotations=sc["rotations"], shs=sc["shs"], viewmatrix=sc["viewmatrix"], projmatrix=sc["projmatrix"],
                campos=sc["campos"], tanfovx=float(sc["tanfovx"]), tanfovy=float(sc["tanfovy"]), W=int(sc["W"]), H=int(sc["H"]),
                sh_degree=int(sc["sh_degree"]), scale_modifier=float(sc.get("scale_modifier", 1.0)))


def oracle_forward(o, a, colors_precomp=None, transMat_precomp=None, depth_key=None, use_sh=True):
    return o.rasterize_forward(a["bg"], a["means3D"], colors_precomp, a["opacities"],
                               None if transMat_precomp is not None else a["scales"],
                               None if transMat_precomp is not None else a["rotations"], a["scale_modifier"],
                               transMat_precomp, a["viewmatrix"], a["projmatrix"], a["tanfovx"], a["tanfovy"], a["H"], a["W"],
                               a["shs"] if (use_sh and colors_precomp is None) else None, a["sh_degree"], a["campos"],
                               depth_key_f32=depth_key)


class HipRun:
    """One forward (+ optional backward) through libsurfel_hip.so's C ABI with torch-owned memory."""

    def __init__(self, a, colors_precomp=None, transMat_precomp=None, debug=False, device="cuda:0"):
        import torch
        import surfel_native as n
        self.n, self.torch, self.dev = n, torch, torch.device(device)
        self.lib = n.load()
        t = lambda x: None if x is None else torch.as_tensor(np.ascontiguousarray(x, dtype=np.float32)).to(self.dev)
        self.a = a
        self.P = a["means3D"].shape[0]
        self.W, self.H, self.D = a["W"], a["H"], a["sh_degree"]
        self.bg, self.means3D, self.opac = t(a["bg"]), t(a["means3D"]), t(a["opacities"])
        self.scales = None if transMat_precomp is not None else t(a["scales"])
        self.rots = None if transMat_precomp is not None else t(a["rotations"])
        self.trans = t(transMat_precomp)
        self.colors = t(colors_precomp)
        self.shs = None if colors_precomp is not None else t(a["shs"])
        self.M = 0 if self.shs is None else self.shs.shape[1]
        self.view, self.proj, self.campos = t(a["viewmatrix"]), t(a["projmatrix"]), t(a["campos"])
        self.debug = int(debug)

    def forward(self):
        torch, n = self.torch, self.n
        self.color = torch.empty((3, self.H, self.W), device=self.dev)
        self.others = torch.empty((7, self.H, self.W), device=self.dev)
        self.radii = torch.full((self.P,), -7, dtype=torch.int32, device=self.dev)
        self.ga, self.ba, self.ia = n.TorchAllocator(self.dev), n.TorchAllocator(self.dev), n.TorchAllocator(self.dev)
        a = self.a
        R = self.lib.surfel_rasterize_forward(self.ga.cb, None, self.ba.cb, None, self.ia.cb, None, self.P, self.D, self.M,
                                              n.ptr(self.bg), self.W, self.H, n.ptr(self.means3D), n.ptr(self.shs),
                                              n.ptr(self.colors), n.ptr(self.opac), n.ptr(self.scales), a["scale_modifier"],
                                              n.ptr(self.rots), n.ptr(self.trans), n.ptr(self.view), n.ptr(self.proj),
                                              n.ptr(self.campos), a["tanfovx"], a["tanfovy"], 0, n.ptr(self.color),
                                              n.ptr(self.others), n.ptr(self.radii), self.debug, n.current_stream_ptr(self.dev))
        self.rc = min(int(R), 0)      # the call's error code (0: none), kept for the tests of refused arguments
        assert R >= 0, "forward failed: %s" % n.last_error()
        self.R = int(R)
        torch.cuda.synchronize()
        return self

    def depths(self):
        """float32 view depths the device sorted on (white-box: geom buffer = [rec P*112 B | depths ...])."""
        off = (self.P * 112 + 255) // 256 * 256
        return self.ga.last()[off:off + 4 * self.P].view(self.torch.float32).cpu().numpy()

    def backward(self, gC, gO, skip=()):
        """skip: names of optional outputs ("normal", "transMat") passed as NULL; they are left out of the returned dict."""
        torch, n = self.torch, self.n
        z = lambda *s: torch.full(s, float('nan'), device=self.dev)   # poison: the kernels must write every element
        P, M = self.P, self.M
        self.g = dict(means2D=z(P, 3), normal=z(P, 3), opacity=z(P, 1), colors=z(P, 3), means3D=z(P, 3), transMat=z(P, 9),
                      sh=z(P, max(M, 1), 3), scales=z(P, 2), rots=z(P, 4))
        gC = torch.as_tensor(np.ascontiguousarray(gC, np.float32)).to(self.dev)
        gO = torch.as_tensor(np.ascontiguousarray(gO, np.float32)).to(self.dev)
        self.sa = n.TorchAllocator(self.dev)
        g, a = self.g, self.a
        rc = self.lib.surfel_rasterize_backward(self.sa.cb, None, P, self.D, M, self.R, n.ptr(self.bg), self.W, self.H,
                                                n.ptr(self.means3D), n.ptr(self.shs), n.ptr(self.colors), n.ptr(self.scales),
                                                a["scale_modifier"], n.ptr(self.rots), n.ptr(self.trans), n.ptr(self.view),
                                                n.ptr(self.proj), n.ptr(self.campos), a["tanfovx"], a["tanfovy"],
                                                n.ptr(self.radii), n.ptr(self.ga.last()), n.ptr(self.ba.last()),
                                                n.ptr(self.ia.last()), n.ptr(gC), n.ptr(gO), n.ptr(g["means2D"]),
                                                None if "normal" in skip else n.ptr(g["normal"]), n.ptr(g["opacity"]), n.ptr(g["colors"]),
                                                n.ptr(g["means3D"]), None if "transMat" in skip else n.ptr(g["transMat"]),
                                                n.ptr(g["sh"]) if M else None, n.ptr(g["scales"]),
                                                n.ptr(g["rots"]), self.debug, n.current_stream_ptr(self.dev))
        self.rc = int(rc)
        assert rc >= 0, "backward failed: %s" % n.last_error()
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in g.items() if k not in skip}


def frac_close(x, ref, atol, rtol):
    x = np.asarray(x, np.float64); ref = np.asarray(ref, np.float64)
    ok = np.abs(x - ref) <= atol + rtol * np.abs(ref)
    return float(ok.mean())


def cosine(x, ref):
    x = np.asarray(x, np.float64).ravel(); ref = np.asarray(ref, np.float64).ravel()
    d = np.linalg.norm(x) * np.linalg.norm(ref)
    return float(x @ ref / d) if d > 0 else 1.0


# The small-scene checks against the fp64 oracle (tests/test_gpu_parity.py states the tolerances; determinacy.py holds the constants).
def check_binning(run, R, radii):
    """Small scenes: radii exact.  The device emits a (tile, surfel) instance only where the surfel's alpha >= 1/255 bbox reaches the
    tile, so its instance count is a subset of the reference rect count the oracle reports.  (Config sizes: determinacy.judge_radii.)"""
    got = run.radii.cpu().numpy()
    assert np.array_equal(got, radii) and run.R <= R, (int((got != radii).sum()), run.R, R)


def image_figures(c, o, col, oth):
    """[(channel name, fraction of pixels within the image tolerance)] of colour [3, H, W] and the allmap [7, H, W] against a reference"""
    import determinacy as D
    rows = [("color", frac_close(c, col, D.IMG_ATOL, D.IMG_RTOL))]
    for ch, nm in [(0, "depth-sum"), (1, "alpha"), (2, "nx"), (3, "ny"), (4, "nz"), (6, "distortion")]:
        rows.append((nm, frac_close(o[ch], oth[ch], D.IMG_ATOL, D.IMG_RTOL)))
    rows.append(("median depth", frac_close(o[5], oth[5], 1e-4, 1e-4)))
    return rows


def check_image_arrays(c, o, col, oth):
    """check_images on host arrays (the plain-fp32 oracle's images are held to the device's bar in tests/test_inputs_cpu.py)"""
    import determinacy as D
    assert np.isfinite(c).all() and np.isfinite(o).all()
    for nm, f in image_figures(c, o, col, oth):
        assert f >= D.PASS_FRAC, "%s: only %.5f of pixels within tolerance" % (nm, f)


def check_images(run, col, oth, st):
    check_image_arrays(run.color.cpu().numpy(), run.others.cpu().numpy(), col, oth)


def oracle_grads(og, has_sr=True):
    """an oracle backward's result under the names HipRun.backward gives its gradients"""
    g = dict(means3D=og.dL_dmeans3D, opacity=og.dL_dopacity, sh=og.dL_dsh, means2D=og.dL_dmean2D)
    if has_sr:
        g.update(scales=og.dL_dscales, rots=og.dL_drots)
    return g


def grad_figures(g, og, has_sr=True):
    """[(name, fraction of elements within the gradient tolerance, surfels with an element outside it, cosine)] against the oracle"""
    import determinacy as D
    rows = []
    for k, ref in oracle_grads(og, has_sr).items():
        x = np.asarray(g[k]).reshape(ref.shape)
        assert np.isfinite(x).all(), k
        scale = np.abs(ref).mean() + 1e-30
        f = frac_close(x, ref, 1e-4 * scale + 1e-12, D.G_RTOL)
        bad = np.abs(x.astype(np.float64) - ref) > (1e-4 * scale + 1e-12 + D.G_RTOL * np.abs(ref))
        rows.append((k, f, int(bad.reshape(bad.shape[0], -1).any(1).sum()), cosine(x, ref)))
    return rows


def check_grads(g, og, has_sr=True):
    """g: gradients by HipRun.backward's names, from the device or (oracle_grads) from another run of the oracle"""
    import determinacy as D
    for k, f, bad_surfels, cs in grad_figures(g, og, has_sr):
        # a (pixel, surfel) pair sitting exactly on the 1/255 or 1e-4 threshold may be decided differently in fp32;
        # that moves ONE surfel's gradient, so small scenes get an absolute allowance of 3 surfels
        assert f >= D.PASS_FRAC or bad_surfels <= 3, "%s: only %.5f of elements within tolerance, %d surfels (cos %.7f)" % (k, f, bad_surfels, cs)
        assert cs >= D.COS_MIN, "%s: cosine %.7f" % (k, cs)
