"""CPU: the ``python -m noisy_src.inference`` entry point around the renderer -- the
reference's flags (inference.py:470-503), ``render_video``'s files and noise order
(inference.py:365-443) alone and sharded over two gloo ranks, and the refusal of CPU
tensors by the fused image tail.  Rendering is replaced by a deterministic stand-in."""
import json
import os
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from noisy_src import inference, metrics
from noisy_src.data import BlenderData
from noisy_src.noise import NoiseConfig, add_noise_to_pose, set_noise_seed

REFERENCE_FLAGS = ["checkpoint", "--mode", "test", "video", "single", "--scene", "--data_root", "--output_dir",
                   "--device", "--rotation_noise", "--translation_noise", "--noise_seed", "--n_frames", "--fps",
                   "--chunk_size"]
NOISE = dict(rotation_noise_deg=2.0, translation_noise=0.05, seed=3)
N_FRAMES, H, W = 5, 8, 6


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _fake_render(renderer, pose, H, W, focal, chunk_size=4096):
    """Deterministic stand-in for the HIP render: a function of the pose only."""
    base = torch.sigmoid(pose[:3, :].sum(0)[:3])
    img = base.view(1, 1, 3).expand(H, W, 3).clone()
    img[::2] *= 0.9
    return {"rgb": img, "depth": torch.linspace(2, 6, H * W).view(H, W), "acc": torch.ones(H, W)}


def _quiet(*_, **__):
    pass


def test_help_lists_every_reference_flag(capsys):
    with pytest.raises(SystemExit) as e:
        inference.main(["--help"])
    assert e.value.code == 0
    text = capsys.readouterr().out
    for flag in REFERENCE_FLAGS + ["--precision", "--image_index"]:
        assert flag in text, flag


def test_parser_defaults_match_reference():
    a = inference.build_arg_parser().parse_args(["ckpt.pt"])
    assert (a.mode, a.scene, a.data_root, a.output_dir, a.device) == ("test", None, None, None, "cuda")
    assert (a.rotation_noise, a.translation_noise, a.noise_seed) == (0.0, 0.0, None)
    assert (a.n_frames, a.fps, a.chunk_size, a.precision, a.image_index) == (120, 30, 4096, None, 0)


def test_render_video_layout(tmp_path, monkeypatch):
    monkeypatch.setattr(inference, "render_image", _fake_render)
    poses = inference.create_spiral_poses(n_frames=N_FRAMES, device="cpu")
    got = inference.render_video(None, poses, H, W, 7.0, tmp_path / "v", NoiseConfig(**NOISE), fps=12, log=_quiet)
    frames = tmp_path / "v" / "frames"
    assert sorted(f.name for f in frames.iterdir()) == [f"frame_{i:04d}.png" for i in range(N_FRAMES)]
    cfg = json.loads((tmp_path / "v" / "video_config.json").read_text())
    assert set(cfg) == {"n_frames", "fps", "noise_config", "timestamp"}
    assert set(cfg["noise_config"]) == {"rotation_noise_deg", "translation_noise", "seed"}
    assert cfg["n_frames"] == N_FRAMES and cfg["fps"] == 12 and cfg["noise_config"]["seed"] == 3
    assert got in (tmp_path / "v" / "video.mp4", frames)
    assert got.exists()


def test_render_video_noise_order(tmp_path, monkeypatch):
    """The frames see the poses of the reference's loop: one seed, then frame by frame."""
    seen = []

    def capture(renderer, pose, *args, **kw):
        seen.append(pose.clone())
        return _fake_render(renderer, pose, *args, **kw)

    monkeypatch.setattr(inference, "render_image", capture)
    poses = inference.create_spiral_poses(n_frames=N_FRAMES, device="cpu")
    inference.render_video(None, poses, H, W, 7.0, tmp_path, NoiseConfig(**NOISE), log=_quiet)
    set_noise_seed(3)
    want = [add_noise_to_pose(poses[i], rotation_noise_deg=2.0, translation_noise=0.05)[0] for i in range(N_FRAMES)]
    assert len(seen) == N_FRAMES
    for a, b in zip(seen, want):
        assert torch.equal(a, b)
    assert not torch.equal(seen[0], poses[0])


def _video_worker(rank, world, port, outdir, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        inference.render_image = _fake_render
        written = []
        real_write = inference.Path.write_text

        def spy(self, *a, **kw):
            written.append(self.name)
            return real_write(self, *a, **kw)

        inference.Path.write_text = spy
        poses = inference.create_spiral_poses(n_frames=N_FRAMES, device="cpu")
        got = inference.render_video(None, poses, H, W, 7.0, outdir, NoiseConfig(**NOISE),
                                     process_group=dist.group.WORLD, log=_quiet)
        out[rank] = (str(got), written)
    finally:
        dist.destroy_process_group()


def test_render_video_two_ranks(tmp_path, monkeypatch):
    monkeypatch.setattr(inference, "render_image", _fake_render)
    poses = inference.create_spiral_poses(n_frames=N_FRAMES, device="cpu")
    inference.render_video(None, poses, H, W, 7.0, tmp_path / "one", NoiseConfig(**NOISE), log=_quiet)
    with mp.Manager() as m:
        out = m.dict()
        mp.spawn(_video_worker, args=(2, _free_port(), str(tmp_path / "two"), out), nprocs=2, join=True)
        res = dict(out)
    names = [f"frame_{i:04d}.png" for i in range(N_FRAMES)]
    assert sorted(f.name for f in (tmp_path / "two" / "frames").iterdir()) == names
    for n in names:
        assert (tmp_path / "two" / "frames" / n).read_bytes() == (tmp_path / "one" / "frames" / n).read_bytes(), n
    assert res[0][1] == ["video_config.json"] and res[1][1] == []
    assert res[0][0] == res[1][0]  # every rank returns rank 0's result


def test_fused_tail_has_no_cpu_fallback(tmp_path, monkeypatch):
    img = torch.rand(8, 6, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics.image_metrics(img, img.clone())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.frame_u8(img)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.depth_frame_u8(img[..., 0])
    monkeypatch.setattr(inference, "render_image", _fake_render)
    g = torch.Generator().manual_seed(7)
    data = BlenderData(images=torch.rand(2, 8, 6, 3, generator=g), poses=torch.eye(4).repeat(2, 1, 1), H=8, W=6,
                       focal=7.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        inference.evaluate_test_set(None, data, tmp_path, NoiseConfig(), device="cpu", log=_quiet, fused_tail=True)


def test_gaussian_window_is_the_outer_product_of_the_1d_weights():
    g = metrics._gaussian_1d(11)
    assert g.dtype == torch.float32 and g.shape == (11,)
    assert torch.equal(metrics._gaussian_window(11), g.outer(g))
