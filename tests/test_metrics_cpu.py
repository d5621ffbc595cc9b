"""CPU checks of the image-quality evaluation (METRICS.md): the torch oracle (tests/metrics_oracle.py) against what the reference's own
lpipsPyTorch / psnr / ssim / metrics.py computed on the seeded pairs (tests/golden/ref_metrics.npz, minted by
tests/golden/make_golden_metrics.py), the rules against literal restatements, the weight loaders, the JSON half of evaluate and the
library surface (header, exports, kernel resources)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import metrics_oracle as O
import metrics_scenes as S

torch = pytest.importorskip("torch")
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "2d-gaussian-splatting_amd")
HEADER = "surfel_metrics.h"


@pytest.fixture(scope="module")
def gold():
    z = np.load(os.path.join(REPO, "tests", "golden", "ref_metrics.npz"))
    assert json.loads(str(z["pairs"])) == json.loads(json.dumps(list(S.PAIRS))), "the fixture was minted from other pairs: run make_golden_metrics.py"
    return z


@pytest.fixture(scope="module")
def oracle_runs():
    return [O.lpips(*S.pair(k), S.weights(), torch.float64) for k in range(len(S.PAIRS))]


def rel(a, b):
    return abs(float(a) - float(b)) / abs(float(b))


# ------------------------------------------------------------------------------------------------ the oracle against the reference
def test_weight_checksum(gold):
    """The seeded stream still gives the weights the fixture was minted with (sums and sampled values, exactly)."""
    assert np.array_equal(S.checksum(), gold["checksum"])
    convs, biases, lins = S.weights()
    assert [tuple(w.shape) for w in convs] == [(co, ci, 3, 3) for ci, co in S.CHANNELS] and all(w.dtype == np.float32 for w in convs)
    assert [l.shape[1] for l in lins] == list(S.TAP_CHANNELS) and min(float(l.min()) for l in lins) >= 0.0


def test_oracle_reproduces_reference(gold, oracle_runs):
    """fp64 on both sides, identical inputs: 1e-12 relative on LPIPS per view and per layer, PSNR (and its mse) and SSIM."""
    for k, r in enumerate(oracle_runs):
        x, y = S.pair(k)
        assert rel(r["total"], gold["lpips"][k]) < 1e-12
        for j in range(5):
            assert rel(r["terms"][j], gold["terms"][k][j]) < 1e-12, (k, j)
        assert rel(O.psnr(x[None], y[None]), gold["psnr"][k]) < 1e-12 and rel(O.mse(x[None], y[None]), gold["mse"][k]) < 1e-12
        assert rel(O.ssim(x, y), gold["ssim"][k]) < 1e-12
    assert gold["e32"].shape == (len(S.PAIRS), 6) and gold["e32"].max() < 1e-5


def test_oracle_reproduces_reference_evaluate(gold):
    """metrics.py::evaluate ran in fp32 on the CPU: the oracle's fp32 run gives its dictionaries key for key; the values agree to
    1e-5 relative (fp32 sums on another CPU may block differently) and the means are the fp32 torch.tensor(list).mean()."""
    res, per = json.loads(str(gold["results_json"])), json.loads(str(gold["per_view_json"]))
    names = [p["name"] for p in S.PAIRS]
    assert list(res) == [S.METHOD] == list(per) and list(res[S.METHOD]) == ["SSIM", "PSNR", "LPIPS"] == list(per[S.METHOD])
    mine = {"SSIM": [], "PSNR": [], "LPIPS": []}
    for k in range(len(S.PAIRS)):
        x, y = S.pair(k)
        mine["SSIM"].append(float(O.ssim(x, y, torch.float32)))
        mine["PSNR"].append(float(O.psnr(x[None], y[None], torch.float32)))
        mine["LPIPS"].append(float(O.lpips(x, y, S.weights(), torch.float32)["total"]))
    for key in mine:
        assert sorted(per[S.METHOD][key]) == names
        for k, n in enumerate(names):
            assert rel(mine[key][k], per[S.METHOD][key][n]) < 1e-5, (key, n)
        assert res[S.METHOD][key] == torch.tensor([per[S.METHOD][key][n] for n in names]).mean().item()


# ------------------------------------------------------------------------------------------------ rules against literal restatements
def test_tap_rule_literal():
    """normalize_activation + (fx - fy)^2 + 1x1 conv + mean((2, 3)), with a pixel of all-zero features in one image and in both."""
    g = torch.Generator().manual_seed(3)
    fx, fy = torch.rand((1, 64, 5, 7), generator=g, dtype=torch.float64), torch.rand((1, 64, 5, 7), generator=g, dtype=torch.float64)
    fx[0, :, 1, 2] = 0
    fx[0, :, 3, 3] = 0
    fy[0, :, 3, 3] = 0
    w = torch.rand((1, 64, 1, 1), generator=g, dtype=torch.float64)

    def normalize_activation(x, eps=1e-10):
        return x / (torch.sqrt(torch.sum(x ** 2, dim=1, keepdim=True)) + eps)

    want = torch.nn.functional.conv2d((normalize_activation(fx) - normalize_activation(fy)) ** 2, w).mean((2, 3), True)
    got = O.tap(fx, fy, w)
    assert tuple(want.shape) == (1, 1, 1, 1) and rel(got, want) < 1e-13
    assert torch.isfinite(got) and float(normalize_activation(fx)[0, :, 3, 3].abs().max()) == 0.0      # 0 / 1e-10 = 0
    # the all-zero pixel of x alone contributes sum_c w_c fy^_c^2
    only = O.tap(fx[:, :, 1:2, 2:3], fy[:, :, 1:2, 2:3], w)
    assert rel(only, (w[0, :, 0, 0] * normalize_activation(fy)[0, :, 1, 2] ** 2).sum()) < 1e-13
    assert float(O.tap(fx[:, :, 3:4, 3:4], fy[:, :, 3:4, 3:4], w)) == 0.0


def test_pool_floor_on_odd_sizes():
    g = torch.Generator().manual_seed(4)
    x = torch.rand((1, 2, 7, 9), generator=g, dtype=torch.float64)
    p = O.pool(x)
    assert tuple(p.shape) == (1, 2, 3, 4)
    want = torch.stack([x[:, :, 0:6:2, 0:8:2], x[:, :, 1:6:2, 0:8:2], x[:, :, 0:6:2, 1:8:2], x[:, :, 1:6:2, 1:8:2]]).max(0).values
    assert torch.equal(p, want)
    shapes = [tuple(f.shape[-2:]) for f in O.features(torch.zeros((1, 3, 37, 53)), *S.weights()[:2])]
    assert shapes == [(37, 53), (18, 26), (9, 13), (4, 6), (2, 3)]


# ------------------------------------------------------------------------------------------------ the host side of surfel_metrics
def _lib():
    return os.path.join(PKG, "lib", "libsurfel_hip.so")


@pytest.fixture(scope="module")
def M():
    if not os.path.exists(_lib()):
        pytest.fail("libsurfel_hip.so not built: run __graft_entry__.build()")
    import surfel_metrics
    return surfel_metrics


@pytest.mark.parametrize("prefix,lin_style", [("features.", "lpips"), ("", "lpips"), ("features.", "renamed")])
def test_weight_loader_key_spellings(M, tmp_path, prefix, lin_style):
    vgg, lin = S.state_dicts(prefix, lin_style)
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "lin.pth")
    w = M.load_lpips_weights(str(tmp_path / "vgg16.pth"), str(tmp_path / "lin.pth"))
    convs, biases, lins = S.weights()
    assert [tuple(t.shape) for t in w.convs] == [(9, max(ci, 4), co) for ci, co in S.CHANNELS]
    for k in (0, 4, 12):      # [tap = ky * 3 + kx][c_in][c_out] is the transpose of [c_out][c_in][ky][kx]; the padded channel is zero
        ci = S.CHANNELS[k][0]
        assert np.array_equal(w.convs[k][:, :ci].numpy(), convs[k].transpose(2, 3, 1, 0).reshape(9, ci, -1))
        assert np.array_equal(w.biases[k].numpy(), biases[k])
    assert float(w.convs[0][:, 3].abs().max()) == 0.0
    for k in range(5):
        assert np.array_equal(w.lins[k].numpy(), lins[k].ravel())


def test_weight_loader_names_the_missing_key(M, tmp_path):
    vgg, lin = S.state_dicts()
    del vgg["features.17.bias"]
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "lin.pth")
    with pytest.raises(KeyError, match=r"features\.17\.bias"):
        M.load_lpips_weights(str(tmp_path / "vgg16.pth"), str(tmp_path / "lin.pth"))
    vgg, lin = S.state_dicts()
    del lin["lin3.model.1.weight"]
    torch.save(vgg, tmp_path / "vgg16.pth")
    torch.save(lin, tmp_path / "lin.pth")
    with pytest.raises(KeyError, match=r"lin3\.model\.1\.weight"):
        M.load_lpips_weights(str(tmp_path / "vgg16.pth"), str(tmp_path / "lin.pth"))
    with pytest.raises(ValueError, match="convolution 2"):
        c, b, l = S.weights()
        M.lpips_weights_from_tensors([torch.from_numpy(w) for w in c[:2] + c[3:4] + c[3:]], [torch.from_numpy(v) for v in b], [torch.from_numpy(v) for v in l])


def test_evaluate_without_weights_writes_null(M, tmp_path, monkeypatch, capsys):
    """The JSON-writing half, the metric functions stubbed (no device): structure, sorted names, fp32 means, "LPIPS": null, and a scene
    that fails is reported with its reason and does not stop the next one."""
    Image = pytest.importorskip("PIL.Image")
    scene = tmp_path / "scene"
    for sub in ("renders", "gt"):
        os.makedirs(scene / "test" / S.METHOD / sub)
        for k, p in reversed(list(enumerate(S.PAIRS))):
            a = S.pair(k)[0 if sub == "renders" else 1]
            Image.fromarray(np.round(a.transpose(1, 2, 0) * 255).astype(np.uint8)).save(str(scene / "test" / S.METHOD / sub / p["name"]), "PNG")
    seen = []
    monkeypatch.setattr(M, "ssim", lambda r, g: seen.append((r, g)) or torch.tensor(0.25 * len(seen)))
    monkeypatch.setattr(M, "psnr", lambda r, g: torch.tensor([[10.0 + len(seen)]]))
    full, per = M.evaluate([str(tmp_path / "missing"), str(scene)], None, device="cpu")
    err = capsys.readouterr().err
    assert "LPIPS" in err and "no weights" in err and "missing" in err and "FileNotFoundError" in err
    res, pv = json.load(open(scene / "results.json")), json.load(open(scene / "per_view.json"))
    assert res == full[str(scene)] and pv == per[str(scene)]
    assert res == {S.METHOD: {"SSIM": 0.375, "PSNR": 11.5, "LPIPS": None}}
    assert pv == {S.METHOD: {"SSIM": {"00000.png": 0.25, "00001.png": 0.5}, "PSNR": {"00000.png": 11.0, "00001.png": 12.0}, "LPIPS": None}}
    assert open(scene / "results.json").read().startswith('{\n "ours_7": {\n  "SSIM"')      # indent=True
    # to_tensor: uint8 / 255, [1, 3, H, W], exactly the generated pair
    r0, g0 = seen[0]
    assert tuple(r0.shape) == (1, 3, 37, 53) and np.array_equal(r0[0].numpy(), S.pair(0)[0]) and np.array_equal(g0[0].numpy(), S.pair(0)[1])


def test_module_has_no_download_path(M):
    src = open(os.path.join(PKG, "surfel_metrics.py")).read()
    for word in ("http", "urllib", "requests", "hub", "download_url"):
        assert word not in src, word


# ------------------------------------------------------------------------------------------------ library surface
def test_metrics_header_exported():
    sys.path.insert(0, PKG)
    if not os.path.exists(_lib()):
        pytest.fail("libsurfel_hip.so not built: run __graft_entry__.build()")
    decl = re.findall(r"^\w[\w\s\*]*?\b(surfel_\w+)\(", open(os.path.join(REPO, "include", HEADER)).read(), re.M)
    assert len(decl) == 6
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib()]).decode()
    exported = set(re.findall(r" T (\w+)$", out, re.M))
    assert set(decl) <= exported, set(decl) - exported
    import surfel_native
    assert sorted(surfel_native.METRICS_EXPORTS) == sorted(decl) == sorted(surfel_native.SIGNATURES[HEADER])
    assert not set(decl) & set(surfel_native.EXPORTS + surfel_native.MESH_EXPORTS + surfel_native.UNBOUNDED_EXPORTS + surfel_native.EVAL_EXPORTS
                               + surfel_native.TNT_EXPORTS)
    lib = surfel_native.load()
    for name in surfel_native.METRICS_EXPORTS:
        assert getattr(lib, name).argtypes is not None, name


def test_metrics_signatures_match_the_header():
    """test_abi_cpu.test_every_signature_matches_its_header, repeated for surfel_metrics.h (every pointer is a device pointer)."""
    import ctypes as C
    import surfel_native as n
    import test_abi_cpu as A
    lib = n.load()
    scalars = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
    returns = {"int": C.c_int, "int64_t": C.c_int64}
    protos, mentions = A._prototypes(HEADER)
    assert len(protos) == mentions == 6
    assert sorted(p[0] for p in protos) == sorted(n.SIGNATURES[HEADER])
    for name, ret, params in protos:
        fn = getattr(lib, name)
        assert fn.restype is returns[ret], (name, ret, fn.restype)
        assert fn.argtypes is not None and len(fn.argtypes) == len(params), (name, fn.argtypes, params)
        for k, ((ctype, pname), at) in enumerate(zip(params, fn.argtypes)):
            where = (name, k, ctype, pname, at)
            if ctype in scalars:
                assert at is scalars[ctype], where
            else:
                assert ctype.endswith("*"), where
                assert (at is n.DevPtr) == (pname != "stream"), where
            assert (at is n.Stream) == (pname == "stream") and (pname != "stream" or k == len(params) - 1), where


def test_metrics_kernels_no_scratch_no_spills():
    sys.path.insert(0, os.path.join(REPO, "scripts"))
    import isa_count
    text = isa_count.assemble("metrics_lpips.hip")
    ks = isa_count.kernels(text)
    names = [k for k in ks if "lpips_" in k or "sq_err" in k]
    assert len(names) == 6, names      # prepare, conv3x3<4>, conv3x3<16>, pool, tap, sq_err
    for k in names:
        assert int(ks[k][1].get("private_segment_fixed_size", 0)) == 0, k
    spills = re.findall(r"\.(?:s|v)gpr_spill_count:\s*(\d+)", text)
    assert len(spills) == 2 * len(names) and all(int(v) == 0 for v in spills), spills
    conv = [k for k in names if "conv3x3_kernelILi16E" in k][0]
    body = "\n".join(ks[conv][0])
    print("lpips_conv3x3_kernel<16>: %d VGPRs (accum offset %d), %d B LDS, %d MFMA" % (
        ks[conv][1].get("next_free_vgpr", 0), ks[conv][1].get("accum_offset", 0), ks[conv][1].get("group_segment_fixed_size", 0),
        body.count("v_mfma_f32_32x32x2_f32")))
    assert body.count("v_mfma_f32_32x32x2_f32") == 9 * 8 * 4      # the whole chunk unrolled: 9 taps x 8 k-steps x 4 accumulators
    assert ks[conv][1].get("next_free_vgpr", 0) <= 256 and ks[conv][1].get("group_segment_fixed_size", 0) <= 80 * 1024      # two workgroups per CU


def test_metrics_refuses_cpu_tensors(M):
    x = torch.zeros((1, 3, 16, 16))
    w = M.lpips_weights_from_tensors(*[[torch.from_numpy(t) for t in ts] for ts in S.weights()])
    crit = M.LPIPS.__new__(M.LPIPS)      # (the constructor would move the weights to a device)
    crit.weights, crit.budget_bytes, crit.timings = w, M.DEFAULT_BUDGET, None
    act = torch.zeros((2, 4, 4, 64))
    for call in (lambda: M.psnr(x, x), lambda: crit(x, x), lambda: crit.layers(x[0], x[0]), lambda: M.ssim(x, x),
                 lambda: M.conv3x3(act, w.convs[1], w.biases[1]), lambda: M.pool(act), lambda: M.tap(act, w.lins[0])):
        with pytest.raises(RuntimeError) as e:
            call()
        assert "tensors must live on a HIP device" in str(e.value)


def test_metrics_budget_is_checked_before_allocating(M):
    """The calls fail before the library touches a device: no allocator exists on this path at all."""
    import ctypes as C
    import surfel_native as n
    assert M.LimitError is n.LimitError
    need = M.workspace_bytes(1060, 1600, 1 << 40)
    act = 2 * 1060 * 1600 * 64 * 4
    assert need == 2 * act + 6 * 1024 * 4 and act % 256 == 0
    assert M.workspace_bytes(1060, 1600, need) == need
    with pytest.raises(n.LimitError, match=r"\(-4\): .*budget"):
        M.workspace_bytes(1060, 1600, need - 1)
    with pytest.raises(n.LimitError, match=r"\(-4\): .*SURFEL_LPIPS_MAX_EDGE"):
        M.workspace_bytes(16385, 16, 1 << 62)
    with pytest.raises(RuntimeError, match=r"\(-1\): .*bad arguments"):
        M.workspace_bytes(0, 16, 1 << 62)
    with pytest.raises(RuntimeError, match=r"\(-1\): .*cin must be 4 or a multiple of 16"):
        n.call(None, "surfel_lpips_conv3x3", 8, 8, 3, 64, C.c_void_p(256), C.c_void_p(512), C.c_void_p(768), C.c_void_p(1024))
    with pytest.raises(RuntimeError, match=r"\(-1\): .*C must be 64, 128, 256 or 512"):
        n.call(None, "surfel_lpips_tap", 8, 8, 96, C.c_void_p(256), C.c_void_p(512), C.c_void_p(768))
