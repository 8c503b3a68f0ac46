"""CPU: the host side of the coarse-to-fine positional encoding (no kernel runs): BARF's
window weights and schedule, the ``--c2f`` / ``--fixed_small_angle`` flags, and the
argument checks and ``state_dict()`` neutrality of ``NeRF.set_pe_window``."""
import pytest
import torch


def test_pe_window_weights_values():
    from noisy_src.train_pose_opt import pe_window_weights
    w = pe_window_weights(3.4, 10)
    assert w[:3] == [1.0, 1.0, 1.0] and w[4:] == [0.0] * 6
    assert abs(w[3] - 0.3454915028125262) < 1e-15
    w = pe_window_weights(1.36, 4)
    assert w[0] == 1.0 and w[2:] == [0.0, 0.0]
    assert abs(w[1] - 0.2871103542174638) < 1e-15
    assert pe_window_weights(0.0, 10) == [0.0] * 10
    assert pe_window_weights(10.0, 10) == [1.0] * 10
    assert pe_window_weights(12.5, 4) == [1.0] * 4


def test_c2f_alpha():
    from noisy_src.train_pose_opt import c2f_alpha
    assert abs(c2f_alpha(2360, 10000, 0.1, 0.5, 10) - 3.4) < 1e-12
    assert c2f_alpha(0, 10000, 0.1, 0.5, 10) == 0.0      # before start: no frequency
    assert c2f_alpha(1000, 10000, 0.1, 0.5, 10) == 0.0
    assert c2f_alpha(5000, 10000, 0.1, 0.5, 10) == 10.0  # from end on: all of them
    assert c2f_alpha(9999, 10000, 0.1, 0.5, 4) == 4.0
    with pytest.raises(ValueError):
        c2f_alpha(1, 10, 0.5, 0.5, 4)


def test_parser_flags_default_off():
    from noisy_src.train_pose_opt import build_arg_parser
    ap = build_arg_parser()
    a = ap.parse_args([])
    assert a.c2f is None and a.fixed_small_angle is False
    a = ap.parse_args(["--c2f", "0.1", "0.5", "--fixed_small_angle"])
    assert a.c2f == [0.1, 0.5] and a.fixed_small_angle is True
    with pytest.raises(SystemExit):
        ap.parse_args(["--c2f", "0.1"])


def test_train_entry_point_has_the_keywords():
    import inspect
    from noisy_src.train_pose_opt import train_with_pose_optimization
    sig = inspect.signature(train_with_pose_optimization)
    assert sig.parameters["c2f"].default is None
    assert sig.parameters["fixed_small_angle"].default is False


def test_set_pe_window_checks_lengths():
    from noisy_src.config import ModelConfig
    from noisy_src.model import NeRF
    net = NeRF(ModelConfig())
    with pytest.raises(ValueError, match="pos"):
        net.set_pe_window([1.0] * 9)
    with pytest.raises(ValueError, match="dir"):
        net.set_pe_window([1.0] * 10, [1.0] * 5)
    with pytest.raises(ValueError, match="pos"):
        net.set_pe_window(torch.ones(11))
    net.set_pe_window([1.0] * 10, torch.ones(4))
    assert net.pe_window() == ([1.0] * 10, [1.0] * 4)
    net.set_pe_window(None, [0.5, 0.0, 0.0, 0.0])
    assert net.pe_window() == (None, [0.5, 0.0, 0.0, 0.0])
    net.set_pe_window(None, None)
    assert net.pe_window() == (None, None)


def test_set_pe_window_refuses_dir_without_view_dirs():
    from noisy_src.config import ModelConfig
    from noisy_src.model import NeRF
    net = NeRF(ModelConfig(use_view_dirs=False))
    with pytest.raises(ValueError, match="view directions"):
        net.set_pe_window(None, [1.0] * 4)
    net.set_pe_window([0.0] * 10)


def test_graphed_trainer_refuses_a_window_first():
    """The fixed-pose graph replay does not stage window weights: refused before anything else
    is touched (no trainer internals needed)."""
    from types import SimpleNamespace
    from noisy_src.config import ModelConfig
    from noisy_src.engine import GraphedTrainer
    from noisy_src.model import NeRF
    net = NeRF(ModelConfig())
    net.set_pe_window([0.5] * 10)
    with pytest.raises(ValueError, match="window"):
        GraphedTrainer(SimpleNamespace(model_coarse=net, model_fine=None), None, None, None)


def test_state_dict_keys_unchanged_by_a_window():
    from noisy_src.config import ModelConfig
    from noisy_src.model import NeRF
    from oracle import refimpl as ref
    cfg = ModelConfig()
    net = NeRF(cfg)
    before = list(net.state_dict())
    net.set_pe_window([1.0, 1.0, 0.5] + [0.0] * 7, [1.0, 0.25, 0.0, 0.0])
    assert list(net.state_dict()) == before == list(ref.NeRF(cfg).state_dict())
    assert not [n for n, _ in net.named_buffers() if "window" in n]
