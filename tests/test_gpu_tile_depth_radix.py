"""GPU tests of the per-tile depth sort's radix classes (csrc/surfel_sort.hip: tile_radix_lds, tile_radix_chunked) — through the debug
entry against numpy's lexsort at every size-class boundary the library reports, and through the forward on a scene whose tiles sit in
the LDS radix class with one beyond the LDS capacity: the three binning settings must agree bit for bit."""
import ctypes as C

import numpy as np
import pytest

from helpers import HipRun, scene_args

pytestmark = pytest.mark.gpu
GAP = 3                    # words between two runs of the point list: they must keep their bits
GAP_BITS = 0xC0FFEE00


def _classes():
    import surfel_native as n
    out = (C.c_int * 6)()
    assert n.call(None, "surfel_debug_tile_depth_sort_classes", out, 6) == 6
    return dict(zip(("radix_min", "cap_small", "cap_large", "small_avg", "class_a", "class_b"), (int(x) for x in out)))


def _run_lengths(cap, c):
    """every boundary of the kernel with LDS capacity `cap`, -1 / 0 / +1, the fixed small sizes and a run of three chunks and a bit"""
    ls = {0, 1, 2, 63, 64, 65, 255, 256, 257, 3 * cap + 17}
    for b in (c["radix_min"], c["class_a"], c["class_b"], c["cap_small"], c["cap_large"], cap):
        ls |= {max(0, b - 1), b, b + 1}
    return sorted(ls)


def _keys(kind, ids_max, rng):
    """the depth-key table (one word per surfel id)"""
    if kind == "random32":
        return rng.integers(0, 1 << 32, ids_max, dtype=np.uint64).astype(np.uint32)
    if kind == "seven":          # long ties: the order inside them must be by id
        return rng.choice(rng.integers(0, 1 << 32, 7, dtype=np.uint64).astype(np.uint32), ids_max)
    if kind == "equal":          # every pass is skipped
        return np.full(ids_max, 0x40A00000, np.uint32)
    if kind.startswith("byte"):  # the keys differ in exactly one byte: three passes are skipped
        b = int(kind[4])
        return (np.uint32(0x3F8A5C71) & ~np.uint32(0xFF << (8 * b))) | (rng.integers(0, 256, ids_max).astype(np.uint32) << np.uint32(8 * b))
    assert kind == "depths"      # float bits of view depths
    return rng.uniform(0.2, 50.0, ids_max).astype(np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def layouts():
    """per kernel: (ranges [tiles, 2], run ids, point-list length); ids ascending inside every run, not contiguous; shared by all cases"""
    c = _classes()
    rng = np.random.default_rng(11)
    out = {}
    for which, cap in (("small", c["cap_small"]), ("large", c["cap_large"])):
        lens = _run_lengths(cap, c)
        ids_max = 4 * max(lens)
        runs = [np.sort(rng.choice(ids_max, L, replace=False)).astype(np.uint32) for L in lens]
        total = sum(lens) + GAP * (len(lens) + 1)
        # the library picks the kernel from instances per tile: empty tiles in between bring the small one's average down
        tiles = len(lens) if which == "large" else max(len(lens), -(-total // c["small_avg"]) + 1)
        assert (total <= c["small_avg"] * tiles) == (which == "small")
        slots = np.sort(rng.choice(tiles, len(lens), replace=False))
        ranges = np.zeros((tiles, 2), np.uint32)
        pos = GAP
        for t, L in zip(slots, lens):
            ranges[t] = (pos, pos + L)
            pos += L + GAP
        out[which] = (ranges, dict(zip((int(t) for t in slots), runs)), total, ids_max, c)
    return out


@pytest.mark.parametrize("decode", [0, 1])
@pytest.mark.parametrize("kind", ["random32", "seven", "equal", "byte0", "byte1", "byte2", "byte3", "depths"])
@pytest.mark.parametrize("which", ["small", "large"])
def test_tile_depth_sort_matches_lexsort(layouts, which, kind, decode):
    """every run comes out as np.lexsort((ids, keys)) orders it; words outside the runs keep their bits; the ranges come back decoded;
    a second call on the output changes nothing"""
    import torch
    import surfel_native as n
    ranges, runs, total, ids_max, c = layouts[which]
    dev = torch.device("cuda:0")
    keys = _keys(kind, ids_max, np.random.default_rng(5))
    pl = np.full(total, GAP_BITS, np.uint32)
    want = pl.copy()
    for t, ids in runs.items():
        s, e = int(ranges[t, 0]), int(ranges[t, 1])
        pl[s:e] = ids
        want[s:e] = ids[np.lexsort((ids, keys[ids]))]
    plain = ranges.copy()
    given = ranges.copy()
    if decode:      # as the capacity path's tile sort leaves them: start complemented, (0, 0) for a tile without instances
        empty = ranges[:, 0] == ranges[:, 1]
        given[:, 0] = ~ranges[:, 0]
        given[empty] = 0
        plain[empty] = 0
    as_dev = lambda x: torch.as_tensor(x.view(np.int32)).to(dev)
    d_rg, d_pl, d_keys = as_dev(given.reshape(-1)), as_dev(pl), as_dev(keys)
    scratch = torch.empty(3 * total, dtype=torch.int32, device=dev)
    tiles = ranges.shape[0]
    assert n.call(dev, "surfel_debug_tile_depth_sort", tiles, total, d_rg, d_pl, d_keys, scratch, decode) == 0
    torch.cuda.synchronize()
    got = d_pl.cpu().numpy().view(np.uint32)
    bad = [(t, int(ranges[t, 1] - ranges[t, 0])) for t in runs if not np.array_equal(got[ranges[t, 0]:ranges[t, 1]], want[ranges[t, 0]:ranges[t, 1]])]
    assert not bad, "runs (tile, length) out of order: %s" % bad
    assert np.array_equal(got, want), "words outside the runs changed"
    assert np.array_equal(d_rg.cpu().numpy().view(np.uint32).reshape(-1, 2), plain), "ranges not decoded"
    assert n.call(dev, "surfel_debug_tile_depth_sort", tiles, total, d_rg, d_pl, d_keys, scratch, 0) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_pl.cpu().numpy().view(np.uint32), want), "a second call changed the order"
    assert np.array_equal(d_rg.cpu().numpy().view(np.uint32).reshape(-1, 2), plain)


def _crowded_scene(ties):
    """64 x 48 pixels = 12 tiles: faint surfels with footprints of a few tiles put a couple of thousand instances on every tile, and a
    bundle of small ones along one ray piles several thousand more onto the tile that ray goes through"""
    import synthetic
    P = 10500
    sc = synthetic.make_scene(P, 64, 48, seed=6, px_radius=5.0, z_near=2.0, z_far=8.0, tilt=False)
    rng = np.random.default_rng(9)
    m = sc["means3D"]
    h = np.concatenate([m, np.ones((m.shape[0], 1), np.float32)], axis=1) @ sc["projmatrix"].reshape(4, 4)      # (row vectors, as torch stores it)
    pix = ((h[:, :2] / h[:, 3:4] + 1.0) * np.array([64, 48]) - 1.0) * 0.5
    ref = int(np.argmin(np.abs(pix - np.array([40.0, 24.0])).sum(axis=1) + 1e3 * (h[:, 3] <= 0)))      # nearest to the centre of tile (2, 1)
    assert np.abs(pix[ref] - np.array([40.0, 24.0])).max() < 3.0
    bundle = rng.permutation(P)[:4500]
    bundle = bundle[bundle != ref]
    assert np.allclose(sc["campos"], 0.0)      # (tilt=False: the camera sits at the origin, so scaling a point keeps its pixel)
    m[bundle] = m[ref][None, :] * rng.uniform(0.7, 1.8, (bundle.size, 1)).astype(np.float32)
    sc["scales"][bundle] *= 0.15
    if ties:      # view depth = world z: quantised, hundreds of surfels share a depth bit pattern
        m[:, 2] = np.round(m[:, 2] * 2.0) / 2.0
    sc["opacities"] = np.full_like(sc["opacities"], 0.02)      # faint: nothing saturates, every instance is blended
    return sc


@pytest.mark.parametrize("ties", [False, True], ids=["crowded", "ties"])
def test_binning_settings_agree_in_the_radix_classes(ties):
    """depth-presorted emission (0) against the per-tile depth sort (2) against the library's rule (1, twice): equal R, radii, images and
    gradients, on a frame where most tiles take the LDS radix and at least one is streamed in chunks"""
    import surfel_native as n
    c = _classes()
    a = scene_args(_crowded_scene(ties))
    rng = np.random.default_rng(3)
    gC = rng.normal(size=(3, a["H"], a["W"])).astype(np.float32); gO = rng.normal(size=(7, a["H"], a["W"])).astype(np.float32)
    res = []
    for mode in (0, 2, 1, 1):
        run = HipRun(a, debug=n.opt_tile_sort(mode)).forward()
        if mode == 2:
            rg = run.ia.last()[:12 * 8].view(run.torch.int32).view(12, 2).cpu().numpy()
            lens = rg[:, 1] - rg[:, 0]
            assert lens.sum() == run.R and run.R > c["small_avg"] * 12
            assert lens.max() > c["cap_large"], "no tile beyond the LDS capacity: %s" % lens.tolist()
            assert ((lens > c["radix_min"]) & (lens <= c["cap_large"])).sum() >= 7, "most tiles should sit in the LDS radix class: %s" % lens.tolist()
        g = run.backward(gC, gO)
        res.append((run.R, run.color.cpu().numpy(), run.others.cpu().numpy(), run.radii.cpu().numpy(), g))
    R0, c0, o0, r0, g0 = res[0]
    for m, (R2, c2, o2, r2, g2) in enumerate(res[1:]):
        assert R0 == R2 and np.array_equal(r0, r2)
        assert np.array_equal(c0, c2) and np.array_equal(o0, o2), "images differ between the binning settings (%d)" % m
        for k in g0:
            assert np.array_equal(g0[k], g2[k]), "dL/d%s differs between the binning settings (%d)" % (k, m)
