"""The codecs' size queries against recorded values (no device is touched).

tests/golden/codec_sizes.json holds what surfel_png_capacity / surfel_png_scratch_bytes, surfel_jpeg_capacity /
surfel_jpeg_scratch_bytes and surfel_jpegdec_scratch_bytes answered before each codec's scratch was described by one carve function
(csrc/carve.h).  It was written once, with the library of that commit, by

    import json, test_codec_sizes_cpu as T
    json.dump(T.sizes(), open("tests/golden/codec_sizes.json", "w"), indent=0, sort_keys=True)

A capacity describes the file and may never change.  A scratch size may not shrink; it may grow by the alignment the carver adds, at
most 16 bytes per carved array.
"""
import json
import os

import jpegdec_scenes as JS

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codec_sizes.json")
PNG_EDGES = (1, 7, 16, 17, 33, 255, 256)
JPEG_EDGES = (1, 15, 16, 17, 33)
PNG_ARRAYS, JPEG_ARRAYS, JPEGDEC_ARRAYS = 8, 4, 17      # arrays carved from each scratch


def sizes():
    import surfel_jpegdec as JD
    import surfel_png as SG
    import surfel_video as SV
    png = [(H, W, Cn) for H in PNG_EDGES for W in PNG_EDGES for Cn in (1, 3)] + [(1080, 1920, 1), (1080, 1920, 3)]
    png.append((1024, (1 << 20) - 1, 1))      # the largest legal frame (test_png_entries_check_their_arguments_without_a_device)
    jpeg = [(H, W) for H in JPEG_EDGES for W in JPEG_EDGES] + [(1080, 1920), (65535, 16)]
    out = {"png": {"%dx%dx%d" % s: [SG.capacity(*s), SG.scratch_bytes(*s)] for s in png},
           "jpeg": {"%dx%d" % s: [SV.capacity(*s), SV.scratch_bytes(*s)] for s in jpeg}, "jpegdec": {}}
    for name in JS.NAMES + ["own-encoder"]:
        data = JS.own_encoder() if name == "own-encoder" else JS.jpeg(name)
        out["jpegdec"][name] = JD.scratch_bytes(JD.parse(data))
    return out


def test_capacities_are_the_recorded_ones_and_scratch_grew_by_alignment_at_most():
    with open(GOLDEN) as f:
        want = json.load(f)
    got = sizes()
    assert {k: sorted(v) for k, v in got.items()} == {k: sorted(v) for k, v in want.items()}
    for codec, arrays in (("png", PNG_ARRAYS), ("jpeg", JPEG_ARRAYS)):
        for key, (cap, scratch) in want[codec].items():
            assert got[codec][key][0] == cap, (codec, key)
            assert scratch <= got[codec][key][1] <= scratch + 16 * arrays, (codec, key, got[codec][key][1], scratch)
    for key, scratch in want["jpegdec"].items():
        assert scratch <= got["jpegdec"][key] <= scratch + 16 * JPEGDEC_ARRAYS, (key, got["jpegdec"][key], scratch)
    assert all(v[1] % 16 == 0 for v in got["png"].values())
