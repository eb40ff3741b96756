"""tests/train_ref.py on the CPU: the torch graph the end-to-end training tests differentiate is the margin loss the loss tests hold the
device to (tests/loss_ref.py), and the layer graph, the comparison rule, the pitched views and the tower twin that the training tests
share do what they say."""
import torch

import loss_ref
import train_ref


def test_margin_loss_f64_is_loss_ref_margin():
    """B = 5, H = 2, d = 8 in float64.  About 100 terms of order 1: a reordered float64 sum moves the result below 1e-13, the
    tolerance is 1e-12 max(1, |loss|).  Seed 0 gives 38.961696565713574 against 38.96169656571358."""
    g = torch.Generator().manual_seed(0)
    s = torch.randn(5, 2, 8, generator=g, dtype=torch.float64)
    im = torch.randn(5, 2, 8, generator=g, dtype=torch.float64)
    got = float(train_ref.margin_loss_f64(s, im, 0.2))
    want = float(loss_ref.margin(s.numpy(), im.numpy(), 0.2, False, 'sum', 'bidir')[0])
    print('train_ref.margin_loss_f64 %r  loss_ref.margin %r' % (got, want))
    assert abs(got - want) <= 1e-12 * max(1.0, abs(want))
    # (B, d) is the one-head case
    flat = float(train_ref.margin_loss_f64(s[:, 0], im[:, 0], 0.2))
    assert flat == float(train_ref.margin_loss_f64(s[:, :1], im[:, :1], 0.2))


def test_layer_graph_is_the_hand_written_graph():
    """(N, Dk, D) = (5, 3, 4) in float64: Linear -> tanh -> a given dropout mask at p = 0.25 -> BatchNorm1d(eps 1e-3, momentum 0.3) in
    training mode, against the same three lines written out.  Sums of at most 5 terms of order 1 in float64: 1e-13 of each tensor's
    largest entry is two orders above any reordering; the mask as a bool array and as a tensor give the same bits."""
    g = torch.Generator().manual_seed(1)
    N, Dk, D, p = 5, 3, 4, 0.25
    W, b = torch.randn(D, Dk, generator=g), torch.randn(D, generator=g)
    x, dE = torch.randn(N, Dk, generator=g), torch.randn(N, D, generator=g)
    keep = torch.rand(N, D, generator=g) >= p
    assert keep.any() and not keep.all()
    got = train_ref.layer_graph(torch.float64, W, b, x, dE, 'tanh', True, keep.numpy(), p, eps=1e-3, momentum=0.3)
    Wd, bd, xd = (t.double().requires_grad_(True) for t in (W, b, x))
    a = torch.tanh(xd @ Wd.T + bd)
    u = a * keep.double() / (1.0 - p)
    y = (u - u.mean(0)) / torch.sqrt(u.var(0, unbiased=False) + 1e-3)                 # gamma 1, beta 0
    y.backward(dE.double())
    want = {'y': y, 'a': a, 'x.grad': xd.grad, 'fc1.weight.grad': Wd.grad, 'fc1.bias.grad': bd.grad,
            'bn1.weight.grad': (dE.double() * y).sum(0), 'bn1.bias.grad': dE.double().sum(0),
            'running_mean': 0.3 * u.mean(0), 'running_var': 0.7 + 0.3 * u.var(0, unbiased=True)}
    assert sorted(got) == sorted(want)
    for k, w in want.items():
        assert got[k].dtype == torch.float64 and float((got[k] - w.detach()).abs().max()) <= 1e-13 * float(w.detach().abs().max()), k
    again = train_ref.layer_graph(torch.float64, W, b, x, dE, 'tanh', True, keep, p, eps=1e-3, momentum=0.3)
    assert all(torch.equal(again[k], got[k]) for k in got)
    # no mask, no BatchNorm: the activation output is y, and the BatchNorm entries are absent
    plain = train_ref.layer_graph(torch.float32, W, b, x, dE, None, False)
    assert sorted(plain) == ['a', 'fc1.bias.grad', 'fc1.weight.grad', 'x.grad', 'y'] and torch.equal(plain['y'], plain['a'])
    assert torch.equal(plain['fc1.bias.grad'], dE.sum(0).double())


def test_compare_holds_the_rule_and_fails_beyond_it():
    """max |got - ref| / max |ref| <= max(4 e32, TOL_UNIT): the floor where the float32 graph is exact, 4 e32 where it is not."""
    import pytest
    ref = {'t': torch.tensor([1.0, -2.0], dtype=torch.float64)}
    exact = {'t': ref['t'].clone()}
    unit = train_ref.TOL_UNIT
    at = lambda rel: {'t': ref['t'] + torch.tensor([0.0, 2.0 * rel], dtype=torch.float64)}      # noqa: E731
    assert train_ref.compare(at(0.5 * unit), ref, exact) == pytest.approx(0.5)
    with pytest.raises(AssertionError):
        train_ref.compare(at(1.01 * unit), ref, exact)
    loose = at(1e-5)                                      # a float32 graph 1e-5 off: the bound is 4e-5
    assert train_ref.compare(at(3.9e-5), ref, loose, 'label') == pytest.approx(0.975)
    with pytest.raises(AssertionError):
        train_ref.compare(at(4.1e-5), ref, loose)
    with pytest.raises(AssertionError):                   # a reference that is zero throughout admits only zeros
        train_ref.compare({'z': torch.tensor([1e-30])}, {'z': torch.zeros(1)}, {'z': torch.zeros(1)})


def test_pitched_views_have_the_layout_they_name():
    """The five layouts on the CPU: pitch, base alignment in floats, a canary row on either side, and untouched_around telling a write
    inside the view from one into the pitch's slack."""
    for layout, ld, off in (('dense', 6, 0), ('pitch4', 12, 0), ('pitch3', 9, 0), ('offset', 12, 1), ('window', 15, 3)):
        assert train_ref.pitch(6, layout) == (ld, off)
        buf, view = train_ref.place(torch.arange(18.0).reshape(3, 6), layout, device='cpu')
        assert view.stride() == (ld, 1) and view.storage_offset() % 4 == off and view.storage_offset() >= ld
        assert buf.numel() >= view.storage_offset() + 3 * ld + ld and torch.equal(view, torch.arange(18.0).reshape(3, 6))
        assert train_ref.untouched_around(buf, view)
        view[2, 5] = 0.0
        assert train_ref.untouched_around(buf, view)
        buf[view.storage_offset() - 1] = 0.0
        assert not train_ref.untouched_around(buf, view)
    for aligned, lo in ((False, 1), (True, 4)):
        buf, view = train_ref.out_vec(7, aligned, device='cpu')
        assert view.storage_offset() == lo and view.numel() == 7 and buf.isnan().all() and buf.numel() == 15


def test_side_f64_leaves_alias_or_copy():
    """side_f64 on a two-projection tower, float64 on the CPU: the leaves carry the module's names; with clone=True they are copies (a
    caller may step them), without it a float64 CPU parameter is aliased; E is the same either way."""
    torch.manual_seed(3)
    side = train_ref.Side((5, 3), 8, 2).double()
    feats = [torch.randn(4, 5, dtype=torch.float64), torch.randn(4, 3, dtype=torch.float64)]
    E, leaves = train_ref.side_f64(side, feats)
    E2, copies = train_ref.side_f64(side, feats, clone=True)
    assert tuple(E.shape) == (4, 2, 4) and torch.equal(E, E2) and sorted(leaves) == sorted(copies)
    assert {'feat0', 'feat1', 'proj.0.fc1.weight', 'proj.1.fc1.bias', 'att.attention_layer.1.embedding_common.0.weight'} <= set(leaves)
    w = side.proj[0].fc1.weight
    assert leaves['proj.0.fc1.weight'].data_ptr() == w.data_ptr() and copies['proj.0.fc1.weight'].data_ptr() != w.data_ptr()
    E.sum().backward()
    assert all(t.grad is not None for t in leaves.values()) and w.grad is None
