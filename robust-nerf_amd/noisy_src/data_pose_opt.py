"""
Pixel batches for joint pose optimisation — drop-in for ShawnnnLiu/Robust-NeRF
``noisy_src/data_pose_opt.py``.

The reference regenerates each batch's rays from the current (learnable) poses with a
Python loop over the unique images of the batch, two ``.item()`` syncs per image and
masked scatters (data_pose_opt.py:83-148).  Here one HIP kernel
(``nr_rays_from_pixels_fwd``) gathers every ray straight from (image, u, v) and its
image's pose, and its backward scatters dL/d(rays_o, rays_d) into dL/d(poses): same
values, same gradient, no host round trips.  Batch assembly is one kernel too
(``nr_gather_pixels``): image index, pixel coordinates and colour from the drawn flat
pixel index, without the reference's two n_pixels-long index tables.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import ops
from .data import BlenderData


@dataclass
class PixelBatch:
    """Reference data_pose_opt.py:21-26."""

    image_indices: torch.Tensor  # (B,) int64
    pixel_coords: torch.Tensor   # (B, 2) float (u, v)
    target_rgb: torch.Tensor     # (B, 3)
    # set by PixelSampler.sample_batch, whose indices are in range by construction;
    # batches built elsewhere are validated (one host sync) before the ray kernel
    in_range: bool = False

    def slice(self, sl: slice) -> "PixelBatch":
        """Rows ``sl`` of the batch (a data-parallel rank's contiguous share)."""
        return PixelBatch(self.image_indices[sl], self.pixel_coords[sl], self.target_rgb[sl], self.in_range)


class PixelDataset:
    """Reference data_pose_opt.py:29-148."""

    def __init__(self, data: BlenderData):
        self.H, self.W, self.focal = data.H, data.W, data.focal
        self.device = data.images.device
        self.n_images = data.images.shape[0]
        # (n_img, H, W, 3) fp32, contiguous: what ``ops.gather_pixels`` reads
        self.images = data.images.float().contiguous()
        self.target_rgb = self.images.reshape(-1, 3)
        self.n_pixels = self.n_images * self.H * self.W
        self.ray_directions = ops.ray_directions(self.H, self.W, self.focal, self.W / 2.0, self.H / 2.0, self.device)
        # the reference's two n_pixels-long tables (data_pose_opt.py:52-70) are pure functions
        # of the index (16 B per pixel: 1 GB at 100 views of 800 x 800); the sampler computes
        # them per batch in its gather kernel, and the attributes are built on first access
        self._image_indices: Optional[torch.Tensor] = None
        self._pixel_coords: Optional[torch.Tensor] = None

    @property
    def image_indices(self) -> torch.Tensor:
        """(n_pixels,) int64: the image of every pixel (built on first access)."""
        if self._image_indices is None:
            self._image_indices = torch.repeat_interleave(
                torch.arange(self.n_images, dtype=torch.long, device=self.device), self.H * self.W)
        return self._image_indices

    @property
    def pixel_coords(self) -> torch.Tensor:
        """(n_pixels, 2) fp32 (u, v) of every pixel (built on first access)."""
        if self._pixel_coords is None:
            v, u = torch.meshgrid(torch.arange(self.H, dtype=torch.float32, device=self.device),
                                  torch.arange(self.W, dtype=torch.float32, device=self.device), indexing="ij")
            single = torch.stack([u.flatten(), v.flatten()], dim=-1)
            self._pixel_coords = single.unsqueeze(0).expand(self.n_images, -1, -1).reshape(-1, 2)
        return self._pixel_coords

    def get_rays_from_pixels(self, pixel_batch: PixelBatch, poses: torch.Tensor,
                             fxy: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Reference data_pose_opt.py:83-148.  ``poses`` holds one pose per UNIQUE image of
        the batch, in ascending image order (``poses_all[torch.unique(indices)]``).
        ``fxy`` (optional, (2,) fp32 device tensor): learnable focal lengths (fx, fy) in place
        of the dataset's ``focal``, or (6,): a lens (fx, fy, cx, cy, k1, k2)
        (``ops.rays_from_pixels``)."""
        uniq, inv = torch.unique(pixel_batch.image_indices, return_inverse=True)
        if poses.shape[0] != uniq.shape[0]:
            raise ValueError(f"get_rays_from_pixels: {poses.shape[0]} poses for {uniq.shape[0]} unique images")
        # ``inv`` indexes ``uniq`` by construction: nothing to validate here
        return ops.rays_from_pixels(inv, pixel_batch.pixel_coords, poses, self.H, self.W,
                                    self.focal if fxy is None else fxy, validate=False)


class PixelSampler:
    """Reference data_pose_opt.py:151-223: uniform pixels with replacement."""

    def __init__(self, dataset: PixelDataset, batch_size: int = 1024):
        self.dataset = dataset
        self.batch_size = batch_size
        self.device = dataset.device
        self.n_pixels = dataset.n_pixels

    def sample_batch(self, generator=None, out=None) -> PixelBatch:
        """``generator`` (optional, on the dataset's device) makes the draw reproducible
        across data-parallel ranks that each take a slice of it.  One kernel
        (``nr_gather_pixels``) turns the drawn indices into the batch: the values of the
        reference's three table gathers, bit for bit.  ``out``: preallocated
        (image_indices, pixel_coords, target_rgb) tensors the kernel writes in place (the
        static inputs of ``graphed.GraphedPoseTrainer``); the batch then holds them."""
        idx = torch.randint(0, self.n_pixels, (self.batch_size,), device=self.device, generator=generator)
        img, pix, rgb = ops.gather_pixels(idx, self.dataset.images, validate=False, out=out)
        return PixelBatch(image_indices=img, pixel_coords=pix, target_rgb=rgb, in_range=True)

    def get_rays_for_batch(self, pixel_batch: PixelBatch, poses: torch.Tensor,
                           fxy: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Reference data_pose_opt.py:200-223 with ``poses`` = every image's pose (N,4,4):
        the kernel indexes them by image directly (the reference's unique/select/loop
        gives the same rays), and the pose gradient lands on every image in the batch.
        ``fxy`` (optional, (2,) fp32 device tensor): learnable focal lengths (fx, fy) in place
        of the dataset's ``focal``, or (6,): a lens (fx, fy, cx, cy, k1, k2); they get a
        gradient too."""
        ds = self.dataset
        return ops.rays_from_pixels(pixel_batch.image_indices, pixel_batch.pixel_coords, poses, ds.H, ds.W,
                                    ds.focal if fxy is None else fxy, validate=not pixel_batch.in_range)


def create_pixel_dataset(data: BlenderData) -> Tuple[PixelDataset, PixelSampler]:
    """Reference data_pose_opt.py:226-241."""
    ds = PixelDataset(data)
    return ds, PixelSampler(ds)
