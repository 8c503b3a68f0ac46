"""Host logic of engine.py and graphed.py that needs no GPU."""

import contextlib

import pytest
import torch
import torch.nn as nn


class _Net(nn.Module):
    """Stand-in with the attributes _adopt_reduced_grad reads: equal-sized parameter sets,
    .grad tensors that are NOT views of the flat gradient (the copy fallback), and the
    last backward's flat gradient."""

    def __init__(self, flat):
        super().__init__()
        self.a = nn.Parameter(torch.zeros(3, 2))
        self.b = nn.Parameter(torch.zeros(4))
        self._param_count = 10
        self._last_gflat = flat
        for p in self.parameters():
            p.grad = torch.full_like(p, -1.0)


def test_reduced_grad_fallback_picks_each_nets_own_flat():
    """Coarse and fine nets have equal parameter counts; with the coarse chain on a second
    stream the coarse all-reduce can be launched first, so the pending list's order says
    nothing about ownership (the copy fallback used to match by size only, and removed
    the match with list.remove, whose == on tensors is elementwise)."""
    from noisy_src.engine import _adopt_reduced_grad
    f_coarse = torch.arange(10, dtype=torch.float32)
    f_fine = torch.arange(10, dtype=torch.float32) + 100
    coarse, fine = _Net(f_coarse), _Net(f_fine)
    flats = [f_fine, f_coarse]  # fine first, as in the one-stream step
    _adopt_reduced_grad(coarse, flats)
    _adopt_reduced_grad(fine, flats)
    assert torch.equal(torch.cat([coarse.a.grad.reshape(-1), coarse.b.grad]), f_coarse)
    assert torch.equal(torch.cat([fine.a.grad.reshape(-1), fine.b.grad]), f_fine)
    assert flats == []


# ------------------------------------------------- graphed._StaticInputs (CPU tensors) --
B, NC, NF = 4, 2, 3  # rays, num_samples, num_samples_fine


def _inputs(t_rand=None, u=None, has_fine=True, **render):
    from noisy_src.config import RenderConfig
    from noisy_src.graphed import _StaticInputs
    rc = RenderConfig(num_samples=NC, num_samples_fine=NF, **render)
    static = [torch.arange(B * 3, dtype=torch.float32).reshape(B, 3) + 100 * k for k in range(3)]
    return _StaticInputs("Holder", static, t_rand, u, rc, has_fine)


def test_static_inputs_predraw_nothing_when_randoms_are_injected():
    t_rand, u = torch.rand(B, NC), torch.rand(B, NF)
    h = _inputs(t_rand, u)
    assert h._predraw == []
    assert torch.equal(h.static_rand[0], t_rand) and h.static_rand[0] is not t_rand  # its own copies
    assert torch.equal(h.static_rand[1], u) and h.static_rand[1] is not u


def test_static_inputs_predraw_both_with_perturb_and_a_fine_net():
    h = _inputs()
    assert [tuple(t.shape) for t in h._predraw] == [(B, NC), (B, NF)]
    assert h._predraw[0] is h.static_rand[0] and h._predraw[1] is h.static_rand[1]
    # drawn with uniform_() in the eager step's order: torch.rand(B, NC), then torch.rand(B, NF)
    torch.manual_seed(3)
    h.draw()
    torch.manual_seed(3)
    assert torch.equal(h.static_rand[0], torch.rand(B, NC)) and torch.equal(h.static_rand[1], torch.rand(B, NF))


def test_static_inputs_predraw_nothing_with_raw_noise():
    h = _inputs(raw_noise_std=1.0)
    assert h._predraw == [] and h.static_rand == [None, None]
    assert _inputs(perturb=False)._predraw == []


def test_static_inputs_predraw_one_without_hierarchical_sampling():
    for h in (_inputs(use_hierarchical=False), _inputs(has_fine=False)):
        assert [tuple(t.shape) for t in h._predraw] == [(B, NC)]
        assert h.static_rand[1] is None


def test_static_inputs_stage_copies_values_and_skips_its_own_buffers():
    t_rand, u = torch.rand(B, NC), torch.rand(B, NF)
    h = _inputs(t_rand, u)
    assert isinstance(h.static, list) and len(h.static) == 3
    srcs = [torch.rand(B, 3) for _ in range(3)]
    t2, u2 = torch.rand(B, NC), torch.rand(B, NF)
    ptrs = [t.data_ptr() for t in h.static + h.static_rand]
    h.stage(srcs, t2, u2)
    for dst, src in zip(h.static + h.static_rand, srcs + [t2, u2]):
        assert torch.equal(dst, src) and dst is not src
    assert [t.data_ptr() for t in h.static + h.static_rand] == ptrs  # in place
    before = [t.clone() for t in h.static + h.static_rand]
    h.stage(h.static, *h.static_rand)  # a buffer onto itself
    h.stage((None, None, None))
    assert all(torch.equal(a, b) for a, b in zip(h.static + h.static_rand, before))


@pytest.mark.parametrize("rows", [1, 5])
def test_static_inputs_stage_refuses_another_shape(rows):
    """(1, 3) for a (4, 3) buffer is the case copy_ would broadcast over the whole batch.
    Nothing is copied by a refused call, not even the valid inputs before the bad one."""
    h = _inputs(torch.rand(B, NC), torch.rand(B, NF))
    before = [t.clone() for t in h.static]
    with pytest.raises(ValueError, match=rf"\({rows}, 3\).*\({B}, 3\)"):
        h.stage((torch.ones(B, 3), torch.ones(rows, 3), None))
    assert all(torch.equal(a, b) for a, b in zip(h.static, before))


def test_static_inputs_stage_refuses_a_random_the_graph_draws():
    h = _inputs(raw_noise_std=1.0)
    with pytest.raises(ValueError, match="drawn in the graph"):
        h.stage((None, None, None), torch.rand(B, NC), torch.rand(B, NF))
    h = _inputs(use_hierarchical=False)  # one pre-drawn buffer: t_rand may be injected, u has no slot
    h.stage((None, None, None), torch.rand(B, NC))
    with pytest.raises(ValueError, match="drawn in the graph"):
        h.stage((None, None, None), None, torch.rand(B, NF))


def test_static_inputs_stage_wants_both_randoms_or_neither():
    h = _inputs()
    for t_rand, u in ((torch.rand(B, NC), None), (None, torch.rand(B, NF))):
        with pytest.raises(ValueError, match="inject both"):
            h.stage((None, None, None), t_rand, u)
    torch.manual_seed(11)
    h.stage((None, None, None))  # neither: drawn here
    torch.manual_seed(11)
    assert torch.equal(h.static_rand[0], torch.rand(B, NC))
    t_rand, u = torch.rand(B, NC), torch.rand(B, NF)
    state = torch.get_rng_state()
    h.stage((None, None, None), t_rand, u)  # both: copied, nothing drawn
    assert torch.equal(h.static_rand[0], t_rand) and torch.equal(h.static_rand[1], u)
    assert torch.equal(torch.get_rng_state(), state)


# ------------------------------------------------------------------ graphed._capture --
class _StubSchedule:
    """Records the calls _capture makes; ``optimizer`` only carries device_sched."""

    def __init__(self, log, name):
        from types import SimpleNamespace
        self.log, self.name, self.pair = log, name, object()
        self.optimizer = SimpleNamespace(device_sched=None)

    def common_step(self):
        self.log.append((self.name, "common_step"))
        return 0

    def snapshot(self):
        self.log.append((self.name, "snapshot"))
        return ("snap", self.name)

    def restore(self, snap):
        self.log.append((self.name, "restore", snap))


@pytest.mark.parametrize("distributed", [False, True])
def test_capture_rolls_back_when_the_step_raises(monkeypatch, distributed):
    """A capture that raises (OOM, a collective that is not capturable) must not leave the
    optimizers reading their device pairs, nor the host bookkeeping advanced."""
    from noisy_src import graphed
    modes = []

    @contextlib.contextmanager
    def no_capture(graph, capture_error_mode):
        modes.append(capture_error_mode)
        yield

    monkeypatch.setattr(graphed.torch.cuda, "CUDAGraph", object)
    monkeypatch.setattr(graphed.torch.cuda, "graph", no_capture)
    log = []
    scheds = [_StubSchedule(log, "nerf"), _StubSchedule(log, "poses")]
    seen = []

    def run_step():
        seen.extend(s.optimizer.device_sched is s.pair for s in scheds)
        raise MemoryError("capture failed")

    with pytest.raises(MemoryError, match="capture failed"):
        graphed._capture(scheds, run_step, distributed)
    assert seen == [True, True]  # the step ran with every optimizer on its pair
    assert modes == ["thread_local" if distributed else "global"]
    for s in scheds:
        assert s.optimizer.device_sched is None
        mine = [e[1:] for e in log if e[0] == s.name]
        assert mine == [("common_step",), ("snapshot",), ("restore", ("snap", s.name))]

    # and the same bracket around a step that succeeds
    del log[:]
    graph, out = graphed._capture(scheds, lambda: "metrics", distributed)
    assert out == "metrics" and all(s.optimizer.device_sched is None for s in scheds)
    assert [e[2] for e in log if e[1] == "restore"] == [("snap", "nerf"), ("snap", "poses")]
