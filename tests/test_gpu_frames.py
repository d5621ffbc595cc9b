"""The slot ring and the device side the two writers share (surfel_frames), through the writers: slots reused by frames of other sizes
grow their buffers, every file is its frame's, every slot comes back."""
import io

import numpy as np
import pytest

import video_oracle as VO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def test_frame_writer_reuses_slots_for_frames_of_other_sizes(tmp_path):
    from PIL import Image
    import surfel_path as SP
    rng = np.random.default_rng(7)
    shapes = [(4, 4, 3), (17, 33, 3), (40, 40, 1), (7, 13, 3), (33, 65, 1), (4, 4, 3)]      # sizes go up and down, gray among RGB
    frames = [rng.integers(0, 256, size=s, dtype=np.uint8) for s in shapes]
    with SP.FrameWriter(workers=2, ring=2, png="device") as fw:
        for k, a in enumerate(frames):
            fw.submit(str(tmp_path / ("%d.png" % k)), _dev(a))
    assert fw.frames == 6
    for k, a in enumerate(frames):
        got = np.asarray(Image.open(io.BytesIO(open(str(tmp_path / ("%d.png" % k)), "rb").read())))
        assert np.array_equal(got[:, :, None] if got.ndim == 2 else got, a), k
    assert sorted(fw._ring._idle) == [0, 1]      # every slot is idle after close()


def test_video_writer_with_one_slot_keeps_submission_order(tmp_path):
    import surfel_video as SV
    rng = np.random.default_rng(8)
    frames = [rng.integers(0, 256, size=(17, 33, 3), dtype=np.uint8) for _ in range(3)]
    host = VO.encode(frames[0][::-1].copy(), 95)      # a JFIF file from the host, between the device frames
    path = str(tmp_path / "one.avi")
    with SV.VideoWriter(path, 17, 33, ring=1) as vw:
        vw.add_frame(_dev(frames[0]))
        vw.add_frame(_dev(frames[1]))
        vw.add_jpeg(host)
        vw.add_frame(_dev(frames[2]))
    assert vw.frames == vw.submitted == 4 and sorted(vw._ring._idle) == [0]
    want = [SV.jpeg_bytes(_dev(f), 95) for f in frames]
    assert VO.read_avi(path)["frames"] == [want[0], want[1], host, want[2]]
