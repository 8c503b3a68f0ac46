"""CPU: the size queries of the frozen-field MLP pair (host code, no kernel launch).

16-bit: ``nr_mlp_frozen_saved_bytes`` is the ReLU mask region alone, ceil(M / 32) tiles x
n_mask KB with no padding tiles; the workspace holds the dz images the input gradients read
(layer 0, the layer after each skip, dir_linear) plus flags and block counts.  For the
default model that is 288 B per sample against about 5.3 KB saved (the test asks 8x, a 2x
margin) and 1.28 KB against 4.9 KB of dz before slabs (the test asks 3x).

The 3x workspace ratio is a property of the DEFAULT model's layer count: a frozen step
stores (kept trunk layers x 512 + 256) B per sample of the training step's
((n + 1) x 512 + 256 + 64) B.  With two skips that is 1792 of 4928 B (2.75x) and with two
layers 768 of 1856 B (2.4x): no layout that keeps what the input-gradient kernel reads
reaches 3x there.  For the other configs the workspace is therefore held to the layout
itself -- at most the kept images over tiles + 64 scratch tiles, the flags, the block counts
and 256-byte alignment -- and to 3x wherever the arithmetic above allows it.
fp32 keeps the training sizes (its backward reads the activations)."""
import ctypes

import pytest

from noisy_src import _hip

M_FINE = 786432  # 4096 rays x 192 samples
CONFIGS = {
    "default": dict(n_layers=8, skip_mask=1 << 4, use_view_dirs=1),
    "no_skip": dict(n_layers=8, skip_mask=0, use_view_dirs=1),
    "skips_2_5": dict(n_layers=8, skip_mask=(1 << 2) | (1 << 5), use_view_dirs=1),
    "no_view_dirs": dict(n_layers=8, skip_mask=1 << 4, use_view_dirs=0),
    "two_layers": dict(n_layers=2, skip_mask=0, use_view_dirs=1),
}
PREC16 = [_hip.NR_PREC_BF16, _hip.NR_PREC_FP16]


def _lib():
    if not _hip.lib_path().exists():
        pytest.skip("library not built (run __graft_entry__.build())")
    return _hip.load()


def _cfg(precision, **kw):
    return _hip.NrMlpConfig(pos_freqs=10, dir_freqs=4, hidden=256, precision=precision, **kw)


def _sizes(L, cfg, M):
    c = ctypes.byref(cfg)
    return (L.nr_mlp_frozen_saved_bytes(c, M), L.nr_mlp_saved_bytes(c, M), L.nr_mlp_frozen_workspace_bytes(c, M),
            L.nr_mlp_workspace_bytes(c, M))


@pytest.mark.parametrize("precision", PREC16)
@pytest.mark.parametrize("name", list(CONFIGS))
def test_16bit_frozen_sizes(name, precision):
    L, kw = _lib(), CONFIGS[name]
    fs, ts, fw, tw = _sizes(L, _cfg(precision, **kw), M_FINE)
    tiles, n_mask = (M_FINE + 31) // 32, kw["n_layers"] + 1
    assert fs == tiles * n_mask * 1024
    assert fs * 8 <= ts
    kept = 1 + bin(kw["skip_mask"]).count("1")  # layer 0 and the layer after each skip
    nseg = (tiles + 255) // 256
    layout = (tiles + 64) * (kept * 16384 + 8192) + nseg * 256 + nseg * 16 + (kept + 3) * 256
    assert 0 < fw <= layout
    assert fw < tw
    # per sample: (kept * 512 + 256) B of ((n + 1) * 512 + 256 + 64) B of training dz
    if 3 * (kept * 512 + 256) <= (kw["n_layers"] + 1) * 512 + 320:
        assert fw * 3 <= tw, (fw, tw)
    if name == "default":
        assert fw * 3 <= tw and fs // tiles == 9 * 1024


@pytest.mark.parametrize("name", list(CONFIGS))
def test_fp32_frozen_sizes_are_at_most_the_training_sizes(name):
    L = _lib()
    for M in (1, 513, M_FINE):
        fs, ts, fw, tw = _sizes(L, _cfg(_hip.NR_PREC_FP32, **CONFIGS[name]), M)
        assert 0 < fs <= ts and 0 < fw <= tw


@pytest.mark.parametrize("precision", PREC16 + [_hip.NR_PREC_FP32])
def test_empty_batch_and_bad_config(precision):
    """M == 0: no saved bytes (16-bit) and a workspace that does not grow with M (the scratch
    tiles alone); M < 0 and a config outside the envelope: -1 with the plan's message."""
    L = _lib()
    cfg = _cfg(precision, **CONFIGS["default"])
    fs0, ts0, fw0, tw0 = _sizes(L, cfg, 0)
    assert 0 <= fs0 <= ts0 and 0 <= fw0 <= tw0
    if precision != _hip.NR_PREC_FP32:
        assert fs0 == 0
        assert fw0 <= 64 * (2 * 16384 + 8192) + 3 * 256  # the scratch tiles of the three images
    assert _sizes(L, cfg, 32)[2] > fw0
    assert L.nr_mlp_frozen_saved_bytes(ctypes.byref(cfg), -1) == -1
    assert L.nr_mlp_frozen_workspace_bytes(ctypes.byref(cfg), -1) == -1
    bad = _hip.NrMlpConfig(pos_freqs=10, dir_freqs=4, hidden=128, n_layers=8, skip_mask=16, use_view_dirs=1,
                           precision=precision)
    assert L.nr_mlp_frozen_saved_bytes(ctypes.byref(bad), 1024) == -1
    assert "hidden_dim" in _hip.last_error()
    assert L.nr_mlp_frozen_workspace_bytes(ctypes.byref(bad), 1024) == -1


def test_sizes_grow_by_whole_tiles():
    L = _lib()
    cfg = _cfg(_hip.NR_PREC_BF16, **CONFIGS["default"])
    s = [_sizes(L, cfg, M)[0] for M in (1, 32, 33, 64, 65)]
    assert s == [9216, 9216, 18432, 18432, 27648]
