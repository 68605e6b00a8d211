"""What exposure.ExposureTable and bilagrid.BilateralGridTable share, through their public API on 'cpu': the
constructor's and check_index's refusals, the identity at the start, zero_grad, and the state_dict round trip.  Nothing is launched."""
import numpy as np
import pytest
import torch

from tests.util import bits

V = 4
GRID = (3, 5, 4)                     # (X, Y, L)


def _make(gs, kind, n_views=V):
    if kind == "exposure":
        return gs.exposure.ExposureTable(n_views, "cpu")
    return gs.bilagrid.BilateralGridTable(n_views, "cpu", shape=GRID)


def _identity(kind):
    eye = torch.eye(3, 4)
    if kind == "exposure":
        return eye.repeat(V, 1, 1)
    X, Y, L = GRID
    return eye.reshape(1, 12, 1, 1, 1).expand(V, 12, L, Y, X).contiguous()


KINDS = ("exposure", "bilagrid")


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("bad", [0, -1, True, 2.0])
def test_n_views_must_be_a_positive_int(gs, kind, bad):
    with pytest.raises(ValueError) as e:
        _make(gs, kind, bad)
    assert str(e.value) == f"n_views must be an integer >= 1, not {bad!r}"


@pytest.mark.parametrize("kind", KINDS)
def test_check_index(gs, kind):
    t = _make(gs, kind)
    for bad in (-1, V, True, 1.0, None):
        with pytest.raises(ValueError) as e:
            t.check_index(bad)
        assert str(e.value) == f"a view's 'idx' must be an integer in [0, {V}), not {bad!r}"
    for good in (0, V - 1, np.int64(2), np.int32(V - 1)):
        got = t.check_index(good)
        assert type(got) is int and got == good


@pytest.mark.parametrize("kind", KINDS)
def test_params_start_at_the_identity_and_zero_grad_clears_grad(gs, kind):
    t = _make(gs, kind)
    want = _identity(kind)
    assert t.n_views == V and t.params.dtype == torch.float32 and t.params.is_contiguous()
    assert tuple(t.params.shape) == tuple(want.shape) and torch.equal(t.params, want)
    assert tuple(t.grad.shape) == tuple(want.shape) and not t.grad.any()
    t.grad.fill_(0.5)
    t.grad[1].fill_(float("nan"))
    t.zero_grad()
    assert not t.grad.any()


@pytest.mark.parametrize("kind", KINDS)
def test_state_dict_round_trips_bit_for_bit(gs, kind):
    a, b = _make(gs, kind), _make(gs, kind)
    g = torch.Generator().manual_seed(7)
    st = a.optimizer._state(a.params)
    with torch.no_grad():
        a.params.add_(torch.randn(a.params.shape, generator=g))
        st["exp_avg"].copy_(torch.randn(a.params.shape, generator=g))
        st["exp_avg_sq"].copy_(torch.rand(a.params.shape, generator=g))
    st["step"] = 5
    sd = a.state_dict()
    assert set(sd) == {"params", "exp_avg", "exp_avg_sq", "step"} and sd["step"] == 5 and type(sd["step"]) is int
    assert sd["params"] is not a.params and sd["exp_avg"] is not st["exp_avg"]          # (copies: a later step does not reach them)
    b.load_state_dict(sd)
    back = b.state_dict()
    for k in ("params", "exp_avg", "exp_avg_sq"):
        assert torch.equal(bits(back[k]), bits(sd[k])), k
    assert back["step"] == 5 and torch.equal(bits(b.params), bits(a.params))


@pytest.mark.parametrize("kind", KINDS)
def test_a_state_of_another_shape_is_refused(gs, kind):
    t, other = _make(gs, kind), _make(gs, kind, V + 1)
    before = t.params.clone()
    with pytest.raises(ValueError) as e:
        t.load_state_dict(other.state_dict())
    assert str(e.value) == f"the state holds a table of {tuple(other.params.shape)}, this one is {tuple(t.params.shape)}"
    assert torch.equal(t.params, before) and t.state_dict()["step"] == 0
