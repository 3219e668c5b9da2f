"""engine.EarlyGrads without a device: who gets the buffers the forward launches wrote, and how often."""
import torch

from gtn_applications_amd import engine as E


def _held(rest=None):
    x, w = torch.zeros(2, 3, requires_grad=True), torch.zeros(4, requires_grad=True)
    dx, dw = torch.ones(2, 3), torch.ones(4)
    return E.EarlyGrads((x, w), (dx, dw), rest), dx, dw


def test_take_refuses_tensors_off_the_device_and_leaves_the_buffers_claimable():
    early, dx, dw = _held()
    assert early.take() is None  # (EagerLoss.backward hands over to float32 device tensors only)
    assert early.dx is dx
    got = early.claim(None)
    assert got[0] is dx and got[1] is dw


def test_claim_returns_the_buffers_once():
    early, dx, dw = _held()
    got = early.claim(None)
    assert len(got) == 2 and got[0] is dx and got[1] is dw
    assert early.dx is None and early.buffers is None  # (taken: no reference left behind)
    assert early.claim(None) is None and early.claim(None, (True, True)) is None
    assert early.take() is None


def test_claim_hands_out_only_what_is_wanted():
    early, dx, dw = _held()
    got = early.claim(None, (False, True))
    assert got[0] is None and got[1] is dw
    assert early.claim(None) is None
    none = E.EarlyGrads((torch.zeros(1),), (None,))
    assert none.dx is None and none.claim(None) == (None,)


def test_rest_runs_exactly_once_with_the_buffers():
    calls = []
    early, dx, dw = _held(lambda gout, bufs: calls.append((gout, bufs)))
    got = early.claim(None)
    assert early.claim(None) is None and early.take() is None
    assert len(calls) == 1 and calls[0][0] is None
    assert calls[0][1] is got and got[0] is dx and got[1] is dw


def test_hold_early_offers_only_on_request():
    early, _, _ = _held()

    class Twice(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, offer):
            E.hold_early(ctx, early, offer)
            return 2 * x

        @staticmethod
        def backward(ctx, g):
            E.check_not_released(ctx)
            return 2 * g, None

    x = torch.ones((), requires_grad=True)
    plain, eager = Twice.apply(x, False), E.make_eager(Twice.apply(x, True))
    assert type(E.make_eager(plain)) is torch.Tensor and type(eager) is E.EagerLoss
    kept, offered = plain.grad_fn, eager.grad_fn
    assert kept.early is early and not hasattr(kept, "eager_take")
    assert offered.early is early and offered.eager_take == early.take and offered._wfl_hooked is False
    offered.register_prehook(lambda go: None)
    assert offered._wfl_hooked is True  # (a hook on the node: EagerLoss.backward stands back)
    E.release_node(offered)
    assert offered.early is None and offered.aux is None and offered.eager_take is None
    try:
        E.check_not_released(offered)
    except RuntimeError as e:
        assert "second time" in str(e)
    else:
        raise AssertionError("a released node must refuse backward")
    E.check_not_released(kept)
