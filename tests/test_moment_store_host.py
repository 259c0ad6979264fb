"""Host side of training from stored VAE moments (latte_amd/moment_store.py, tools/train.py: MomentClips): the
row arithmetic, every refusal, the file round trip, and the data class drawing what RawClips draws.  No GPU, no VAE."""
import importlib.util
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from latte_amd import LatteError, MomentStore
from latte_amd.video_transforms import frame_indices

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (9, 14, 30)


def coded_store(planes=2, dtype=torch.float32, lengths=LENGTHS, h=2, w=4):
    """A store whose every row holds its own (clip, frame, plane) as the value 100 clip + frame + 0.5 plane (exact in f16)."""
    clips = []
    for c, t in enumerate(lengths):
        v = 100.0 * c + torch.arange(t, dtype=torch.float32)[:, None] + 0.5 * torch.arange(planes, dtype=torch.float32)[None, :]
        clips.append(v[:, :, None, None, None].expand(t, planes, 8, h, w).to(dtype).contiguous())
    return MomentStore(clips, [f"{c + 1}_clip{c}" for c in range(len(lengths))])


def decode(store, rows):
    """(clip, frame, plane) of each row from the coded content."""
    v = store._data[torch.from_numpy(np.asarray(rows))][:, 0, 0].double()
    clip = (v // 100).long()
    rest = v - 100 * clip
    return clip.tolist(), rest.floor().long().tolist(), ((rest - rest.floor()) > 0.25).tolist()


def test_rows_are_offset_plus_frame_indices():
    s = coded_store()
    first = np.concatenate([[0], np.cumsum(LENGTHS)[:-1]])
    for clip, t in enumerate(LENGTHS):
        for nf, iv in ((4, 1), (4, 2), (3, 3), (1, 1)):
            for start in (0, (t - nf * iv) // 2, t - nf * iv):     # the start, the middle, the last legal start
                for flip in (False, True):
                    got = s.rows(clip, start, flip, nf, iv)
                    want = (first[clip] + frame_indices(start, start + nf * iv, nf)) * 2 + int(flip)
                    assert got.dtype == np.int64 and np.array_equal(got, want), (clip, nf, iv, start, flip)
                    c, f, p = decode(s, got)
                    assert c == [clip] * nf and f == frame_indices(start, start + nf * iv, nf).tolist() and p == [flip] * nf
    one = coded_store(planes=1)
    assert np.array_equal(one.rows(1, 2, False, 4, 3), LENGTHS[0] + frame_indices(2, 14, 4))
    assert s.num_rows == 2 * sum(LENGTHS) and one.num_rows == sum(LENGTHS)


def test_properties():
    s = coded_store(dtype=torch.float16)
    assert s.num_clips == 3 and s.clip_frames == list(LENGTHS) and s.labels == [1, 2, 3] and s.planes == (False, True)
    assert s.dtype == "f16" and s.nbytes == 2 * sum(LENGTHS) * 8 * 8 * 2 and s.latent_hw == (2, 4)
    one = coded_store(planes=1)
    assert one.planes == (False,) and one.dtype == "fp32" and one.nbytes == sum(LENGTHS) * 8 * 8 * 4


def test_refusals():
    s, one = coded_store(), coded_store(planes=1)
    with pytest.raises(LatteError, match="one plane"):
        one.rows(0, 0, True, 4, 1)
    with pytest.raises(LatteError, match="leaves clip"):
        s.rows(0, 2, False, 4, 2)                                 # [2, 10) of a 9-frame clip
    with pytest.raises(LatteError, match="leaves clip"):
        s.rows(0, -1, False, 4, 1)
    for clip in (-1, 3):
        with pytest.raises(LatteError, match="outside the store's 3 clips"):
            s.rows(clip, 0, False, 4, 1)
    with pytest.raises(LatteError):
        s.rows(0, 0, False, 0, 1)
    with pytest.raises(LatteError, match="leave clip"):
        s.frame_rows(0, [0, 9])
    with pytest.raises(LatteError, match="exactly one"):
        s.sample_clips([0], [0], [False], 4, 1)
    with pytest.raises(LatteError, match="exactly one"):
        s.sample_frames([0], seed=1, noise=torch.zeros(1, 4, 2, 4))
    with pytest.raises(LatteError, match="one entry per clip"):
        s.sample_clips([0, 1], [0], [False, False], 4, 1, seed=1)
    with pytest.raises(LatteError):                               # a shape that is not [T, P, 8, h, w]
        MomentStore([torch.zeros(3, 2, 4, 2, 4)], ["a"])
    with pytest.raises(LatteError):                               # clips of different latent sizes
        MomentStore([torch.zeros(3, 2, 8, 2, 4), torch.zeros(3, 2, 8, 4, 4)], ["a", "b"])
    if not torch.cuda.is_available():                             # sampling needs the GPU: LatteError, never a fallback
        with pytest.raises(LatteError, match="MI355X"):
            s.sample_clips([0], [0], [False], 4, 1, seed=1)
        with pytest.raises(LatteError, match="MI355X"):
            s.moments([0])
        with pytest.raises(LatteError, match="MI355X"):
            s.to("cuda")


@pytest.mark.parametrize("dtype", [torch.float32, torch.float16])
@pytest.mark.parametrize("planes", [1, 2])
def test_save_load_round_trip(tmp_path, dtype, planes):
    g = torch.Generator().manual_seed(7)
    clips = [torch.randn(t, planes, 8, 2, 4, generator=g).to(dtype) for t in (3, 5, 2)]
    names = ["4_b", "0_a", "nolabel"]
    s = MomentStore(clips, names)
    s.save(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["0_a.npy", "4_b.npy", "nolabel.npy"]
    assert np.load(tmp_path / "4_b.npy").shape == (3, planes, 8, 2, 4)
    back = MomentStore.load(str(tmp_path), device="cpu")
    assert back.names == ["0_a", "4_b", "nolabel"] and back.labels == [0, 4, 0] and back.clip_frames == [5, 3, 2]
    assert back.planes == s.planes and back.dtype == s.dtype and back.nbytes == s.nbytes and back.device.type == "cpu"
    want = torch.cat([clips[1], clips[0], clips[2]]).reshape(-1, 8, 8)
    assert back._data.dtype == dtype and torch.equal(back._data, want)
    with pytest.raises(LatteError, match="no .npy"):
        MomentStore.load(str(tmp_path / "missing"), device="cpu")


def _train_tool():
    spec = importlib.util.spec_from_file_location("_train_tool_moments", os.path.join(ROOT, "tools", "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_moment_clips_draw_what_raw_clips_draw(tmp_path):
    """Raw clips whose frame j is filled with j on the left half and 255 - j on the right; a store whose rows encode (clip, frame,
    plane).  For several (step, micro, rank) the rows MomentClips picks name the frames RawClips.batch gathers and the flips it draws."""
    train = _train_tool()
    lengths = (9, 14, 30)
    for c, t in enumerate(lengths):
        a = np.zeros((t, 4, 6, 3), dtype=np.uint8)
        a[:, :, :3] = np.arange(t, dtype=np.uint8)[:, None, None, None]
        a[:, :, 3:] = 255 - np.arange(t, dtype=np.uint8)[:, None, None, None]
        np.save(tmp_path / f"{c + 1}_clip{c}.npy", a)
    store = coded_store(lengths=lengths)
    args = SimpleNamespace(dataset="ucf101", num_frames=4, frame_interval=2, image_size=128)
    seen_flips, seen_clips = set(), set()
    for rank, world, accum in ((0, 1, 1), (1, 2, 1), (0, 1, 3)):
        raw = train.RawClips(str(tmp_path), args, rank, world, seed=3407)
        mom = train.MomentClips(store, args, rank, world, seed=3407)
        raw.accum = mom.accum = accum
        assert [os.path.splitext(os.path.basename(f))[0] for f in raw.files] == store.names
        for step in (1, 2, 7):
            for micro in range(accum):
                items, y = raw.batch(step, 5, micro)
                picks, ym = mom.batch(step, 5, micro)
                assert torch.equal(y, ym)
                for (frames, flip), (clip, idx, mflip), label in zip(items, picks, y.tolist()):
                    assert label == clip + 1 and flip == mflip
                    assert frames[:, 0, 0, 0].tolist() == list(idx) and frames[:, 0, 5, 0].tolist() == [255 - j for j in idx]
                    c, f, p = decode(store, store.frame_rows(clip, idx, mflip))
                    assert c == [clip] * 4 and f == frames[:, 0, 0, 0].tolist() and p == [flip] * 4
                    seen_flips.add(flip)
                    seen_clips.add(clip)
    assert seen_flips == {False, True} and seen_clips == {0, 1, 2}
    # the single images of joint training: the indices ImageFrames draws
    img_dir = tmp_path / "imgs"
    img_dir.mkdir()
    for c in range(5):
        np.save(img_dir / f"{c}_img.npy", np.full((4, 2, 2), float(c), dtype=np.float32))
    frames = train.ImageFrames(str(img_dir), 3, 2, 0, 1, 3407, 5)
    istore = MomentStore([torch.full((1, 1, 8, 2, 2), float(c)) for c in range(5)], [f"{c}_img" for c in range(5)])
    mframes = train.MomentFrames(istore, 3, 0, 1, 3407)
    for step in (1, 5):
        x, y = frames.batch(step, 4)
        rows, ym = mframes.batch(step, 4)
        assert torch.equal(y, ym) and rows.tolist() == x[:, :, 0, 0, 0].reshape(-1).long().tolist()


def test_encode_clips_help_lists_moments():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "encode_clips.py"), "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--moments" in r.stdout and "--dtype" in r.stdout, r.stdout + r.stderr
