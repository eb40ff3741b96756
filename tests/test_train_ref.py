"""tests/train_ref.py against tests/loss_ref.py on the CPU: the torch graph the end-to-end training tests differentiate is the margin
loss the loss tests hold the device to."""
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
