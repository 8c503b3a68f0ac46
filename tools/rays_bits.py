"""One SHA-256 per output array of the ray and positional-encoding entry points of rays.hip.

Loads the library that NR_HIP_LIB names (default: the tree's build), runs the entry points
below on fixed seeded inputs and prints ``<case> <sha256>`` lines.  Run it once per library,
each in a fresh process, and diff the two outputs: a refactor of rays.hip changes no line.

    NR_HIP_LIB=/path/to/parent.so python tools/rays_bits.py > parent.txt
    python tools/rays_bits.py > tree.txt && diff parent.txt tree.txt

Cases: nr_ray_directions(_xy) at 5x7 and 33x20 (fx == fy and fx != fy); nr_get_rays_bwd at
N = 1, 255, 257 and 70 000 (past 256 x 256, so the grid-stride loop wraps) with g_ro, g_rd or
both and with or without g_dirs; nr_rays_from_pixels_(intr_)fwd/bwd at B = 1, 255, 257, 1000 and
n_img = 1, 3, 300 (300: the focal partials' stride loop wraps) with one image that has no ray,
an out-of-range image index (unvalidated forward), g_rd NULL, fx == fy and fx != fy, and the
intrinsics backward at B = 0; the four positional-encoding entry points at M = 37, C = 1 and 3,
L = 1, 4 and 10, both include_input, both log_sampling, the window null, all ones and a ramp
from 0.  Where the library has the lens entries (one built before them prints every other line
all the same): nr_ray_directions_lens and nr_rays_from_pixels_lens_fwd/bwd in the same cases,
at a neutral lens (fx != fy, centred, k = 0) and a live one.  Output buffers start as NaN
(accumulated ones as zero).  There is no CPU path."""
import hashlib
import itertools
import sys
from pathlib import Path

import torch

ROOT = Path(__file__).resolve().parents[1]
sys.path[:0] = [str(ROOT), str(ROOT / "robust-nerf_amd")]
DEV = "cuda"
NAN = float("nan")


def main() -> int:
    if not torch.cuda.is_available():
        raise SystemExit("rays_bits: no GPU found (there is no CPU path)")
    from noisy_src import _hip
    from noisy_src._hip import call, ptr

    lib = _hip.load(require_all=False)  # a library of before the lens entries loads too
    has_lens = hasattr(lib, "nr_rays_from_pixels_lens_fwd")
    lenses = (("lens_neutral", (7.3, 5.9, 3.5, 2.5, 0.0, 0.0)), ("lens_live", (7.3, 5.9, 3.2, 2.9, 0.11, -0.03)))
    stream = _hip.stream_ptr()
    print(f"# {_hip.lib_path().name}", file=sys.stderr)

    def emit(case, **arrays):
        for name, t in arrays.items():
            print(f"{case}/{name} {hashlib.sha256(t.cpu().contiguous().numpy().tobytes()).hexdigest()}")

    def nans(*shape):
        return torch.full(shape, NAN, device=DEV)

    def rand(gen, *shape):
        return torch.randn(*shape, generator=gen).to(DEV)

    # ---- ray direction tables
    for H, W in ((5, 7), (33, 20)):
        d = nans(H, W, 3)
        call("nr_ray_directions", H, W, 7.3, W / 2.0, H / 2.0, ptr(d), stream)
        emit(f"ray_directions/{H}x{W}", dirs=d)
        for fx, fy in ((7.3, 7.3), (7.3, 5.9)):
            d = nans(H, W, 3)
            call("nr_ray_directions_xy", H, W, fx, fy, W / 2.0, H / 2.0, ptr(d), stream)
            emit(f"ray_directions_xy/{H}x{W}/fx{fx}_fy{fy}", dirs=d)
        for tag, lens in lenses if has_lens else ():
            d = nans(H, W, 3)
            call("nr_ray_directions_lens", H, W, *lens[:2], W / 2.0 - 3.5 + lens[2], H / 2.0 - 2.5 + lens[3], *lens[4:],
                 ptr(d), stream)
            emit(f"ray_directions_lens/{H}x{W}/{tag}", dirs=d)

    # ---- get_rays backward
    ws = torch.empty(int(lib.nr_get_rays_bwd_workspace_bytes()), device=DEV, dtype=torch.uint8)
    for N in (1, 255, 257, 70000):
        gen = torch.Generator().manual_seed(N)
        dirs, c2w, g_ro, g_rd = rand(gen, N, 3), rand(gen, 4, 4), rand(gen, N, 3), rand(gen, N, 3)
        for which, want_dirs in (("ro", False), ("rd", False), ("rd", True), ("both", False), ("both", True)):
            g_c2w = torch.zeros(4, 4, device=DEV)
            g_dirs = nans(N, 3) if want_dirs else None
            call("nr_get_rays_bwd", ptr(dirs), ptr(c2w), N, ptr(g_ro) if which != "rd" else None,
                 ptr(g_rd) if which != "ro" else None, ptr(g_dirs), ptr(g_c2w), ptr(ws), stream)
            out = {"g_c2w": g_c2w}
            if want_dirs:
                out["g_dirs"] = g_dirs
            emit(f"get_rays_bwd/N{N}/{which}{'+g_dirs' if want_dirs else ''}", **out)

    # ---- rays from pixels, fixed focal length and learned intrinsics
    H, W = 5, 7
    focals = (("focal7.3", 7.3), ("fxy7.3_7.3", (7.3, 7.3)), ("fxy7.3_5.9", (7.3, 5.9)))

    def pixels_fwd(case, img, pix, poses, B, n_img):
        for tag, f in focals:
            ro, rd = nans(B, 3), nans(B, 3)
            if isinstance(f, float):
                call("nr_rays_from_pixels_fwd", ptr(img), ptr(pix), ptr(poses), n_img, H, W, f, B, ptr(ro), ptr(rd),
                     None, stream)
            else:
                fxy = torch.tensor(f, device=DEV)
                call("nr_rays_from_pixels_intr_fwd", ptr(img), ptr(pix), ptr(poses), n_img, H, W, ptr(fxy), B, ptr(ro),
                     ptr(rd), None, stream)
            emit(f"{case}/fwd/{tag}", rays_o=ro, rays_d=rd)
        for tag, f in lenses if has_lens else ():
            ro, rd, lens = nans(B, 3), nans(B, 3), torch.tensor(f, device=DEV)
            call("nr_rays_from_pixels_lens_fwd", ptr(img), ptr(pix), ptr(poses), n_img, H, W, ptr(lens), B, ptr(ro),
                 ptr(rd), None, stream)
            emit(f"{case}/fwd/{tag}", rays_o=ro, rays_d=rd)

    def pixels_bwd(case, img, pix, poses, B, n_img, g_ro, g_rd):
        for tag, f in focals:
            g_poses = torch.zeros(n_img, 4, 4, device=DEV)
            if isinstance(f, float):
                call("nr_rays_from_pixels_bwd", ptr(img), ptr(pix), ptr(poses), n_img, H, W, f, B, ptr(g_ro), ptr(g_rd),
                     ptr(g_poses), stream)
                emit(f"{case}/bwd/{tag}", g_poses=g_poses)
            else:
                fxy = torch.tensor(f, device=DEV)
                fws = nans(int(lib.nr_rays_from_pixels_intr_bwd_workspace_bytes(n_img)) // 4)
                g_fxy = nans(2)
                call("nr_rays_from_pixels_intr_bwd", ptr(img), ptr(pix), ptr(poses), n_img, H, W, ptr(fxy), B,
                     ptr(g_ro), ptr(g_rd), ptr(g_poses), ptr(g_fxy), ptr(fws), stream)
                emit(f"{case}/bwd/{tag}", g_poses=g_poses, g_fxy=g_fxy)
        for tag, f in lenses if has_lens else ():
            g_poses, g_lens, lens = torch.zeros(n_img, 4, 4, device=DEV), nans(6), torch.tensor(f, device=DEV)
            lws = nans(int(lib.nr_rays_from_pixels_lens_bwd_workspace_bytes(n_img)) // 4)
            call("nr_rays_from_pixels_lens_bwd", ptr(img), ptr(pix), ptr(poses), n_img, H, W, ptr(lens), B, ptr(g_ro),
                 ptr(g_rd), ptr(g_poses), ptr(g_lens), ptr(lws), stream)
            emit(f"{case}/bwd/{tag}", g_poses=g_poses, g_lens=g_lens)

    for B, n_img in itertools.product((1, 255, 257, 1000), (1, 3, 300)):
        gen = torch.Generator().manual_seed(1000 * B + n_img)
        pool = torch.tensor([i for i in range(n_img) if i != 1 or n_img == 1])  # image 1 has no ray
        img = pool[torch.randint(0, len(pool), (B,), generator=gen)].to(DEV)
        pix = torch.stack([torch.randint(0, W, (B,), generator=gen), torch.randint(0, H, (B,), generator=gen)],
                          -1).float().to(DEV)
        poses, g_ro, g_rd = rand(gen, n_img, 4, 4), rand(gen, B, 3), rand(gen, B, 3)
        case = f"rays_from_pixels/B{B}/n_img{n_img}"
        pixels_fwd(case, img, pix, poses, B, n_img)
        bad = img.clone()
        bad[B // 2] = n_img  # out of range: NaN rays (the forward without validation only)
        pixels_fwd(case + "/bad_index", bad, pix, poses, B, n_img)
        pixels_bwd(case, img, pix, poses, B, n_img, g_ro, g_rd)
        pixels_bwd(case + "/g_rd_null", img, pix, poses, B, n_img, g_ro, None)
    for n_img in (1, 3):  # the empty batch: g_fxy written as zeros, g_poses untouched
        g_poses, g_fxy = torch.zeros(n_img, 4, 4, device=DEV), nans(2)
        fxy = torch.tensor((7.3, 5.9), device=DEV)
        fws = nans(int(lib.nr_rays_from_pixels_intr_bwd_workspace_bytes(n_img)) // 4)
        call("nr_rays_from_pixels_intr_bwd", None, None, None, n_img, H, W, ptr(fxy), 0, None, None, ptr(g_poses),
             ptr(g_fxy), ptr(fws), stream)
        emit(f"rays_from_pixels/B0/n_img{n_img}/bwd/fxy7.3_5.9", g_poses=g_poses, g_fxy=g_fxy)
        if has_lens:
            g_poses, g_lens, lens = torch.zeros(n_img, 4, 4, device=DEV), nans(6), torch.tensor(lenses[1][1], device=DEV)
            lws = nans(int(lib.nr_rays_from_pixels_lens_bwd_workspace_bytes(n_img)) // 4)
            call("nr_rays_from_pixels_lens_bwd", None, None, None, n_img, H, W, ptr(lens), 0, None, None, ptr(g_poses),
                 ptr(g_lens), ptr(lws), stream)
            emit(f"rays_from_pixels/B0/n_img{n_img}/bwd/lens_live", g_poses=g_poses, g_lens=g_lens)

    # ---- positional encoding, plain and windowed
    M = 37
    for C, L, inc, logs in itertools.product((1, 3), (1, 4, 10), (0, 1), (0, 1)):
        gen = torch.Generator().manual_seed(100 * C + L)
        x = torch.rand(M, C, generator=gen) * 16 - 8
        x[:, 0] = torch.where(torch.arange(M) % 2 == 0, 1e4, -1e4)  # one column far outside
        x = x.to(DEV)
        D = inc + 2 * L
        g = rand(gen, M, C * D)
        case = f"positional_encoding/C{C}/L{L}/inc{inc}/logs{logs}"
        out, gx = nans(M, C * D), nans(M, C)
        call("nr_positional_encoding", ptr(x), M, C, L, inc, logs, ptr(out), stream)
        call("nr_positional_encoding_bwd", ptr(x), M, C, L, inc, logs, ptr(g), ptr(gx), stream)
        emit(case + "/plain", out=out, g_x=gx)
        windows = (("null", None), ("ones", torch.ones(L, device=DEV)),
                   ("ramp", torch.linspace(0, 1, L).to(DEV)))
        for tag, w in windows:
            out, gx = nans(M, C * D), nans(M, C)
            call("nr_positional_encoding_windowed", ptr(x), M, C, L, inc, logs, ptr(w), ptr(out), stream)
            call("nr_positional_encoding_windowed_bwd", ptr(x), M, C, L, inc, logs, ptr(w), ptr(g), ptr(gx), stream)
            emit(f"{case}/window_{tag}", out=out, g_x=gx)
    torch.cuda.synchronize()
    return 0


if __name__ == "__main__":
    sys.exit(main())
