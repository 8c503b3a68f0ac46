"""GPU: entry points of rays.hip that promise each other's bits, compared through the C ABI.

* The plain positional encoding, the windowed one with a null window and the windowed one with
  an all-ones window: forward and backward equal as int32 views (a weight of 1.0f is exact).
* ``nr_get_rays_bwd`` against ``nr_rays_from_pixels_bwd`` on one image, with the table of
  ``nr_ray_directions`` gathered at the pixels: the 12 pose-gradient entries equal as int32
  views.  At N = B <= 256 both kernels give thread t exactly ray t and reduce through the same
  tree; the final kernel of ``nr_get_rays_bwd`` then adds 255 exact zeros.  Above 256 rays the
  two reductions legitimately differ in order, so the test stays at or below it.

Shapes: M = 37 rows (not a multiple of the wave), inputs in +-8 and one column of +-1e4;
H x W = 33 x 20 for the pixels.  Outputs start as NaN, accumulated ones as zero."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.mark.parametrize("logs", [0, 1])
@pytest.mark.parametrize("inc", [0, 1])
@pytest.mark.parametrize("L", [1, 4, 10])
@pytest.mark.parametrize("C", [1, 3])
def test_plain_encoding_equals_windowed_with_null_and_unit_window(C, L, inc, logs):
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    M, D = 37, inc + 2 * L
    gen = torch.Generator().manual_seed(100 * C + L)
    x = torch.rand(M, C, generator=gen) * 16 - 8
    x[:, 0] = torch.where(torch.arange(M) % 2 == 0, 1e4, -1e4)
    x, g = x.to(DEV), torch.randn(M, C * D, generator=gen).to(DEV)
    stream = _hip.stream_ptr()

    def run(entry, *window):
        out, gx = torch.full((M, C * D), NAN, device=DEV), torch.full((M, C), NAN, device=DEV)
        call(entry, ptr(x), M, C, L, inc, logs, *window, ptr(out), stream)
        call(entry + "_bwd", ptr(x), M, C, L, inc, logs, *window, ptr(g), ptr(gx), stream)
        assert torch.isfinite(out).all() and torch.isfinite(gx).all()
        return _bits(out), _bits(gx)

    plain = run("nr_positional_encoding")
    ones = torch.ones(L, device=DEV)
    for window in (None, ptr(ones)):
        out, gx = run("nr_positional_encoding_windowed", window)
        assert torch.equal(out, plain[0]) and torch.equal(gx, plain[1])


@pytest.mark.parametrize("N", [1, 64, 256])
def test_get_rays_bwd_equals_rays_from_pixels_bwd_on_one_image(N):
    from noisy_src import _hip
    from noisy_src._hip import call, ptr
    H, W, focal = 33, 20, 21.7
    gen = torch.Generator().manual_seed(N)
    pose = torch.eye(4)
    pose[:3, :3] = torch.linalg.qr(torch.randn(3, 3, generator=gen))[0]
    pose[:3, 3] = torch.randn(3, generator=gen)
    pose = pose.to(DEV)
    u, v = torch.randint(0, W, (N,), generator=gen), torch.randint(0, H, (N,), generator=gen)
    pix = torch.stack([u, v], -1).float().to(DEV)
    g_ro, g_rd = torch.randn(N, 3, generator=gen).to(DEV), torch.randn(N, 3, generator=gen).to(DEV)
    stream = _hip.stream_ptr()

    table = torch.full((H, W, 3), NAN, device=DEV)
    call("nr_ray_directions", H, W, focal, W / 2.0, H / 2.0, ptr(table), stream)
    dirs = table[v.to(DEV), u.to(DEV)].contiguous()
    g_c2w = torch.zeros(4, 4, device=DEV)
    ws = torch.empty(int(_hip.load().nr_get_rays_bwd_workspace_bytes()), device=DEV, dtype=torch.uint8)
    call("nr_get_rays_bwd", ptr(dirs), ptr(pose), N, ptr(g_ro), ptr(g_rd), None, ptr(g_c2w), ptr(ws), stream)

    img = torch.zeros(N, dtype=torch.int64, device=DEV)
    g_poses = torch.zeros(1, 4, 4, device=DEV)
    call("nr_rays_from_pixels_bwd", ptr(img), ptr(pix), ptr(pose), 1, H, W, focal, N, ptr(g_ro), ptr(g_rd),
         ptr(g_poses), stream)

    assert g_c2w[:3].abs().min() > 0  # all 12 entries are live
    assert torch.equal(_bits(g_c2w[:3]), _bits(g_poses[0, :3]))
    assert torch.count_nonzero(g_c2w[3]) == 0 and torch.count_nonzero(g_poses[0, 3]) == 0
