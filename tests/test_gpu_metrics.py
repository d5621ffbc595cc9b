"""GPU checks of the image-quality evaluation (METRICS.md): single layers, pool and tap against the fp64 oracle (tests/metrics_oracle.py),
the whole LPIPS, PSNR and SSIM against what the reference computed on the seeded pairs (tests/golden/ref_metrics.npz), bit
reproducibility, evaluate / main end to end, export_image and the byte budget.  The shapes are the smallest at which the kernels can
still go wrong: K = 27 padded to 36, images smaller than the 16 x 16 tile, one pixel past a tile edge in both directions, more than one
workgroup, every tap width (16, 32 and 64 lanes per pixel, one and two float4 per lane)."""
import json
import os
import types

import numpy as np
import pytest

import metrics_oracle as O
import metrics_scenes as S

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def M():
    import surfel_metrics
    return surfel_metrics


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(REPO, "tests", "golden", "ref_metrics.npz"))
    assert np.array_equal(S.checksum(), z["checksum"]), "the seeded weights drifted from the fixture's"
    return z


@pytest.fixture(scope="module")
def weights(M, torch):
    """The seeded weights in the library's layout, on the device; shared and never modified."""
    return M.lpips_weights_from_tensors(*[[torch.from_numpy(t) for t in ts] for ts in S.weights()]).to(torch.device("cuda"))


@pytest.fixture(scope="module")
def criterion(M, weights):
    return M.LPIPS(weights, "cuda")


@pytest.fixture(scope="module")
def pairs(torch):
    return [tuple(torch.from_numpy(a).cuda() for a in S.pair(k)) for k in range(len(S.PAIRS))]


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


def nhwc(t):
    """[2, C, H, W] -> the library's [2, H, W, C]"""
    return t.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ single layers
LAYERS = [(0, 37, 53), (2, 19, 23), (8, 5, 7), (8, 2, 3), (5, 33, 65)]      # (index into the 13 convolutions, H, W)


@pytest.mark.parametrize("k,H,W", LAYERS, ids=["3to64_37x53", "64to128_19x23", "512to512_5x7", "512to512_2x3", "256to256_33x65"])
def test_conv_layer_against_fp64(M, torch, weights, k, H, W):
    """max |ours - fp64| <= 4 * 3.5e-7 * max_pixel sum |a . b|, border and interior pixels separately (a wrong halo shows only on the
    border); bias and ReLU both active."""
    cin, cout = S.CHANNELS[k]
    w, b = (torch.from_numpy(t[k]).double() for t in S.weights()[:2])
    g = torch.Generator().manual_seed(100 + k)
    x = torch.randn((2, cin, H, W), generator=g, dtype=torch.float32)
    want = O.conv_relu(x.double(), w, b)
    bound = 4 * 3.5e-7 * float(O.conv_abs(x.double(), w, b).max())
    xin = x if cin != 3 else torch.cat([x, torch.zeros((2, 1, H, W))], 1)
    got = M.conv3x3(nhwc(xin).cuda(), weights.convs[k], weights.biases[k]).cpu().permute(0, 3, 1, 2).double()
    assert tuple(got.shape) == tuple(want.shape)
    assert float((want == 0).double().mean()) > 0.1 and float((want > 0).double().mean()) > 0.1 and float(b.abs().min()) > 0      # ReLU and bias active
    assert torch.equal(got == 0, want == 0) or float(((got == 0) != (want == 0)).double().mean()) < 1e-3      # (a value within rounding of 0)
    border = torch.zeros((H, W), dtype=torch.bool)
    border[0, :] = border[-1, :] = border[:, 0] = border[:, -1] = True
    err = (got - want).abs()
    eb, ei = float(err[:, :, border].max()), float(err[:, :, ~border].max()) if H > 2 and W > 2 else 0.0
    print("conv %d->%d at %dx%d: border %.3g interior %.3g allowed %.3g (ratio %.3f)" % (cin, cout, H, W, eb, ei, bound, max(eb, ei) / bound))
    assert eb <= bound and ei <= bound


@pytest.mark.parametrize("H,W", [(7, 9), (8, 8)])
def test_pool_bit_for_bit(M, torch, H, W):
    g = torch.Generator().manual_seed(H)
    x = torch.randn((2, 64, H, W), generator=g, dtype=torch.float32)
    got = M.pool(nhwc(x).cuda()).cpu().permute(0, 3, 1, 2)
    assert torch.equal(got, torch.nn.functional.max_pool2d(x, 2, 2))


@pytest.mark.parametrize("C", [64, 128, 256, 512])
def test_tap_against_fp64(M, torch, C):
    """One pixel all-zero in x only, one in both.  Bound: a length-C fp32 sum in any order errs by at most (C - 1) 2^-24 of the sum
    of its terms' magnitudes; that happens twice (the norm, the weighted sum), and divisions, the subtraction and the square add a
    handful more: (2 C + 16) 2^-24 of mean_pixels sum_c w_c (|fx^_c| + |fy^_c|)^2, which bounds every term's magnitude."""
    g = torch.Generator().manual_seed(C)
    f = torch.rand((2, C, 5, 7), generator=g, dtype=torch.float32)
    f[0, :, 1, 2] = 0
    f[:, :, 3, 3] = 0
    lin = torch.rand((C,), generator=g, dtype=torch.float32) * (2.0 / C)
    fx, fy = f[0:1].double(), f[1:2].double()
    want = float(O.tap(fx, fy, lin.double()))
    nx = fx / (fx.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    ny = fy / (fy.pow(2).sum(1, keepdim=True).sqrt() + 1e-10)
    scale = float((((nx.abs() + ny.abs()) ** 2) * lin.double().reshape(1, -1, 1, 1)).sum(1).mean())
    bound = (2 * C + 16) * 2.0 ** -24 * scale
    got = float(M.tap(nhwc(f).cuda(), lin.cuda()))
    print("tap C=%d: |ours - fp64| %.3g allowed %.3g (ratio %.4f)" % (C, abs(got - want), bound, abs(got - want) / bound))
    assert np.isfinite(got) and abs(got - want) <= bound
    # the pixel that is zero in both images contributes exactly 0; the one zero in x alone contributes sum_c w_c fy^_c^2
    one = f[:, :, 3:4, 3:4].contiguous()
    assert float(M.tap(nhwc(one).cuda(), lin.cuda())) == 0.0
    one = f[:, :, 1:2, 2:3].contiguous()
    assert rel(M.tap(nhwc(one).cuda(), lin.cuda()), (lin.double() * ny[0, :, 1, 2] ** 2).sum()) <= (2 * C + 16) * 2.0 ** -24


# ------------------------------------------------------------------------------------------------ the whole LPIPS
@pytest.mark.parametrize("k", range(len(S.PAIRS)))
def test_lpips_against_reference_golden(criterion, gold, pairs, k):
    """Each layer term: relative error <= max(16 e32_layer, 2e-6); the total: <= max(16 e32_total, 1e-6)."""
    x, y = pairs[k]
    terms = criterion.layers(x, y).cpu().double().numpy()
    total = float(criterion(x[None], y[None]))
    assert tuple(criterion(x, y).shape) == (1, 1, 1, 1)
    e32 = gold["e32"][k]
    for j in range(5):
        err, allowed = rel(terms[j], gold["terms"][k][j]), max(16 * e32[j], 2e-6)
        print("pair %d layer %d: term %.9g relative error %.3g allowed %.3g (ratio %.3f)" % (k, j + 1, terms[j], err, allowed, err / allowed))
    err, allowed = rel(total, gold["lpips"][k]), max(16 * e32[5], 1e-6)
    print("pair %d total: %.9g relative error %.3g allowed %.3g (ratio %.3f)" % (k, total, err, allowed, err / allowed))
    for j in range(5):
        assert rel(terms[j], gold["terms"][k][j]) <= max(16 * e32[j], 2e-6), j
    assert err <= allowed


def test_lpips_same_bits_twice(criterion, torch, pairs):
    x, y = pairs[0]
    assert float(criterion(x, x)) == 0.0 and float(criterion.layers(y, y).abs().max()) == 0.0
    a, b = criterion.layers(x, y), criterion.layers(x, y)
    assert torch.equal(a, b) and torch.equal(criterion(x, y), criterion(x, y))
    # the tap is symmetric: at most 1 ulp per layer term
    c = criterion.layers(y, x)
    ulp = torch.from_numpy(np.spacing(a.cpu().numpy())).to(a.device)
    assert bool(((a - c).abs() <= ulp).all()), (a, c)


def test_lpips_refuses_small_and_mismatched_images(criterion, torch):
    with pytest.raises(ValueError, match="H, W >= 16"):
        criterion(torch.zeros((3, 15, 40), device="cuda"), torch.zeros((3, 15, 40), device="cuda"))
    with pytest.raises(ValueError):
        criterion(torch.zeros((3, 16, 40), device="cuda"), torch.zeros((3, 16, 41), device="cuda"))
    assert float(criterion(torch.zeros((3, 16, 16), device="cuda"), torch.zeros((1, 3, 16, 16), device="cuda")[0])) == 0.0


def test_lpips_limit_error_before_allocating(M, torch, weights, pairs):
    x, y = pairs[1]
    need = M.workspace_bytes(64, 96, 1 << 40)
    assert float(M.LPIPS(weights, "cuda", budget_bytes=need)(x, y)) > 0
    short = M.LPIPS(weights, "cuda", budget_bytes=need - 1)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(M.LimitError, match="budget"):
        short(x, y)
    assert torch.cuda.memory_allocated() == before


# ------------------------------------------------------------------------------------------------ PSNR and SSIM
@pytest.mark.parametrize("k", range(len(S.PAIRS)))
def test_psnr_ssim_against_reference_golden(M, gold, pairs, k):
    """SSIM at the tolerance test_l1_ssim_match_reference_golden uses (2e-5); PSNR as 1e-6 relative on the mse."""
    x, y = pairs[k]
    m, p, s = M.mse(x[None], y[None]), M.psnr(x[None], y[None]), M.ssim(x[None], y[None])
    assert tuple(p.shape) == (1, 1) and tuple(m.shape) == (1, 1)
    print("pair %d: mse relative error %.3g, psnr %.7f vs %.7f, ssim error %.3g" % (k, rel(m, gold["mse"][k]), float(p), gold["psnr"][k],
                                                                                    abs(float(s) - gold["ssim"][k])))
    assert rel(m, gold["mse"][k]) <= 1e-6
    assert rel(10.0 ** (-float(p) / 10.0), gold["mse"][k]) <= 1e-6
    assert abs(float(s) - gold["ssim"][k]) < 2e-5
    assert tuple(M.psnr(x, y).shape) == (3, 1)      # a [3,H,W] input is a batch of three, as in the reference


# ------------------------------------------------------------------------------------------------ evaluate end to end
def test_evaluate_end_to_end(M, torch, gold, tmp_path, capsys):
    Image = pytest.importorskip("PIL.Image")
    scene = tmp_path / "scene"
    for sub in ("renders", "gt"):
        os.makedirs(scene / "test" / S.METHOD / sub)
    for k, p in enumerate(S.PAIRS):
        for a, sub in zip(S.pair(k), ("renders", "gt")):
            Image.fromarray(np.round(a.transpose(1, 2, 0) * 255).astype(np.uint8)).save(str(scene / "test" / S.METHOD / sub / p["name"]), "PNG")
    vgg, lin = S.state_dicts()
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "vgg.pth")
    assert M.main(["-m", str(scene), "--vgg16", str(tmp_path / "vgg16.pth"), "--lpips_lin", str(tmp_path / "vgg.pth")]) == 0
    res, per = json.load(open(scene / "results.json")), json.load(open(scene / "per_view.json"))
    gres, gper = json.loads(str(gold["results_json"])), json.loads(str(gold["per_view_json"]))
    names = [p["name"] for p in S.PAIRS]
    assert list(res) == list(gres) and list(per) == list(gper)
    assert list(res[S.METHOD]) == list(gres[S.METHOD]) and list(per[S.METHOD]) == list(gper[S.METHOD])
    for key in ("SSIM", "PSNR", "LPIPS"):
        assert list(per[S.METHOD][key]) == names and sorted(gper[S.METHOD][key]) == names
        assert res[S.METHOD][key] == torch.tensor([per[S.METHOD][key][n] for n in names]).mean().item()
    for k, n in enumerate(names):
        assert rel(per[S.METHOD]["LPIPS"][n], gold["lpips"][k]) <= max(16 * gold["e32"][k][5], 1e-6)
        assert rel(10.0 ** (-per[S.METHOD]["PSNR"][n] / 10.0), gold["mse"][k]) <= 1e-6
        assert abs(per[S.METHOD]["SSIM"][n] - gold["ssim"][k]) < 2e-5
    capsys.readouterr()
    assert M.main(["-m", str(scene)]) == 0
    assert "no weights" in capsys.readouterr().err
    res2, per2 = json.load(open(scene / "results.json")), json.load(open(scene / "per_view.json"))
    assert res2[S.METHOD]["LPIPS"] is None and per2[S.METHOD]["LPIPS"] is None
    for key in ("SSIM", "PSNR"):
        assert res2[S.METHOD][key] == res[S.METHOD][key] and per2[S.METHOD][key] == per[S.METHOD][key]


# ------------------------------------------------------------------------------------------------ export_image
def test_export_image(torch, tmp_path):
    """renders/%05d.png and gt/%05d.png, quantised as save_img_u8: NaN -> 0, clip to [0, 1], times 255, truncated."""
    Image = pytest.importorskip("PIL.Image")
    from surfel_mesh import GaussianExtractor
    known = [0.0, 1.0, 0.5, 0.25, 0.999, float("nan"), -0.3, 1.7]
    bytes_ = [0, 255, 127, 63, 254, 0, 0, 255]
    g = torch.Generator().manual_seed(5)
    ex = GaussianExtractor.__new__(GaussianExtractor)
    ex.rgbmaps, ex.viewpoint_stack, expect = [], [], []
    for i in range(2):
        maps = []
        for c in (3, 4):      # the render has 3 channels, original_image 4 (an alpha plane that is not written)
            t = torch.rand((c, 6, 8), generator=g) * 1.2 - 0.1
            t[0, 0, :] = torch.tensor(known)
            maps.append(t)
        ex.rgbmaps.append(maps[0].cuda())
        ex.viewpoint_stack.append(types.SimpleNamespace(original_image=maps[1].cuda()))
        expect.append([(np.clip(np.nan_to_num(m[:3].permute(1, 2, 0).numpy()), 0.0, 1.0) * 255.0).astype(np.uint8) for m in maps])
    ex.export_image(str(tmp_path / "out"))
    assert sorted(os.listdir(tmp_path / "out")) == ["gt", "renders"]
    for sub, j in (("renders", 0), ("gt", 1)):
        assert sorted(os.listdir(tmp_path / "out" / sub)) == ["00000.png", "00001.png"]
        for i in range(2):
            a = np.asarray(Image.open(str(tmp_path / "out" / sub / ("%05d.png" % i))))
            assert a.shape == (6, 8, 3) and a.dtype == np.uint8 and np.array_equal(a, expect[i][j])
            assert a[0, :, 0].tolist() == bytes_
