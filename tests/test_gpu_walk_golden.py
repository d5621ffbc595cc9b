"""-m gpu: the contribution pass and the label pass against recorded bytes.  Both passes accumulate integers with commutative, associative
operations, so their results do not depend on the order of workgroups: "the walk computes what it computed" is an equality of bytes.
tests/golden/walk_digests.json holds the SHA-256 of every result array, recorded by this module's own main:

    python tests/test_gpu_walk_golden.py --record <commit the library was built from>

The scenes are those of tests/test_gpu_contrib.py (partial tiles; lists longer than a staging batch that end inside a batch; a 50 x 37
frame); the label images those of tests/select_scenes.py at one K per LDS bucket, on both sides of a bucket edge.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if __name__ == "__main__":
    for p in (os.path.dirname(HERE), os.path.join(os.path.dirname(HERE), "2d-gaussian-splatting_amd"), HERE):
        sys.path.insert(0, p)

import contrib_scenes as CS
import select_scenes as S
from helpers import HipRun, scene_args

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(HERE, "golden", "walk_digests.json")
SCENES = ["random40", "long", "frame50x37"]
KS = [2, 8, 9, 32]      # one per LDS bucket (K <= 2, <= 8, <= 32), and both sides of the edge between the last two
ARRAYS = ["sum_q", "hits_q", "max_bits", "dominant_q", "views_q", "stamp", "dominant_id"]


def sha(t):
    return hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()


_frames, _golden = {}, {}


def frame(name):
    """(HipRun, the buffers dict add_view takes) of a named scene: one exactly counted forward, rendered once"""
    if name not in _frames:
        import surfel_native as n
        sc, cols, _ = CS.random_scene(6, 40, W=50, H=37) if name == "frame50x37" else CS.ORACLE_SCENES[name]()
        run = HipRun(scene_args(sc), colors_precomp=CS.colors_of(sc, cols), debug=n.OPT_EXACT_BINNING | n.OPT_NO_STREAM).forward()
        _frames[name] = (run, dict(geom=run.ga.last(), binning=run.ba.last(), image=run.ia.last(), num_rendered=run.R, P=run.P, width=run.W, height=run.H))
    return _frames[name]


def contribution_digests(name):
    import surfel_prune as SP
    run, view = frame(name)
    c = SP.Contribution(run.P, DEV)
    dom = c.add_view(view, dominant_id=True)
    assert [f for f, _ in SP._FIELDS] == ARRAYS[:6]
    d = {"contribution/%s/%s" % (name, f): sha(getattr(c, f)) for f in ARRAYS[:6]}
    d["contribution/%s/dominant_id" % name] = sha(dom)
    assert int(c.hits_q.sum()) > 0
    return d


def votes_digests(name, K):
    import torch
    import surfel_select as SS
    run, view = frame(name)
    d = {}
    for what in sorted(S.PATTERNS):
        L = S.PATTERNS[what](run.W, run.H, K)
        lv = SS.LabelVotes(run.P, K, DEV)
        lv.add_view(view, torch.from_numpy(np.ascontiguousarray(L, np.uint8)).to(DEV))
        assert int(lv.votes.sum()) > 0
        d["votes/%s/%s/K%d" % (name, what, K)] = sha(lv.votes)
    return d


def golden():
    if not _golden:
        with open(GOLDEN) as f:
            _golden.update(json.load(f))
    return _golden


def check(got):
    g = golden()
    for key, digest in got.items():
        assert key in g, "no recorded digest for %s" % key
        assert digest == g[key], key


@pytest.mark.parametrize("name", SCENES)
def test_contribution_arrays_keep_their_bytes(name):
    got = contribution_digests(name)
    assert len(got) == 7
    check(got)


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("name", SCENES)
def test_votes_keep_their_bytes(name, K):
    got = votes_digests(name, K)
    assert len(got) == len(S.PATTERNS) == 4
    check(got)


def test_every_recorded_digest_is_checked():
    keys = set(golden()) - {"recorded_at"}
    want = {"contribution/%s/%s" % (n, a) for n in SCENES for a in ARRAYS} | {"votes/%s/%s/K%d" % (n, w, K) for n in SCENES for w in S.PATTERNS for K in KS}
    assert keys == want and "recorded_at" in golden()


def main(argv):
    if len(argv) != 2 or argv[0] != "--record":
        sys.exit(__doc__)
    out = {"recorded_at": "the library of commit %s (loaded through SURFEL_LIB), on an MI355X, by `python tests/test_gpu_walk_golden.py --record`" % argv[1]}
    for name in SCENES:
        out.update(contribution_digests(name))
        for K in KS:
            out.update(votes_digests(name, K))
    with open(GOLDEN, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("recorded %d digests in %s" % (len(out) - 1, GOLDEN))


if __name__ == "__main__":
    main(sys.argv[1:])
