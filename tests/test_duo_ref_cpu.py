"""tests/duo_ref.py on the CPU: the closed form of DuoRec's fused contrastive section is float64 autograd of the reference's
info_nce called twice, the float32-torch yardsticks of both input families stay within half of what the kernel is held to
(DESIGN.md 4.15's rule), and B = 1 gives exact zeros."""
import pytest
import torch

from tests import duo_ref as R

PIN_B = (1, 2, 17, 65)


@pytest.mark.parametrize("B", PIN_B)
def test_restatement_is_float64_autograd_of_info_nce_twice(B):
    for d, temp, family in ((64, 1.0, R.contested), (128, 0.2, R.contested), (64, 1.0, R.peaked)):
        a, p, q = family(B, d)
        for scales in ((1.0, 1.0), (0.1, 0.1), (-2.5, 1.0)):
            ref = R.duo(a, p, q, 1.0 / temp, *scales)
            losses, g = R.duo_autograd(a, p, q, temp, *scales)
            top = max(1.0, float(losses.abs().max()))
            assert float((ref["losses"] - losses).abs().max()) <= 1e-13 * top, (B, d, temp, scales)
            # against what cancels in a gradient row (a peaked row's own size is the rounding of that cancellation)
            z = torch.cat((a, p, q))
            assert R.cancel_figure(g, ref, z, 1.0 / temp, scales, B) <= 1e-13, (B, d, temp, scales)


def test_single_pair_is_exact_zeros():
    for d in R.WIDTHS:
        a, p, q = R.contested(1, d)
        ref = R.duo(a, p, q, 2.0, 0.1, 0.3)
        assert float(ref["losses"].abs().max()) == 0.0 and float(ref["g"].abs().max()) == 0.0
        assert torch.equal(ref["terms"], torch.zeros_like(ref["terms"]))


def test_contested_float32_torch_stays_within_half_the_bounds():
    worst_loss, worst_row, smallest = 0.0, 0.0, float("inf")
    for B in R.CONTESTED_B:
        for d in R.WIDTHS:
            for temp in R.CONTESTED_TEMPS:
                a, p, q = R.contested(B, d)
                ref = R.reference("contested", B, d, temp)
                smallest = min(smallest, float(ref["losses"].min()))
                losses, g = R.duo_autograd(a, p, q, temp, dtype=torch.float32)
                worst_loss = max(worst_loss, *R.rel_loss_figures(losses, ref))
                worst_row = max(worst_row, R.grad_figure(g, ref))
    print(f"contested: float32 torch loss {worst_loss:.3g}, gradient rows {worst_row:.3g} at floor {R.FLOOR_FRAC}; "
          f"smallest loss {smallest:.3g}")
    assert smallest > 0.01                   # every softmax is contested: each loss has a scale of its own
    assert worst_loss <= R.LOSS_TOL / 2 and worst_row <= R.GRAD_TOL / 2


def test_peaked_float32_torch_stays_within_half_the_bounds():
    worst_loss, worst_grad, margin = 0.0, 0.0, float("inf")
    for B in (17, 64, 257):
        a, p, q = R.peaked(B, 64)
        z = torch.cat((a, p, q))
        assert float((z.norm(dim=1) - 8.0).abs().max()) < 1e-4
        ref = R.reference("peaked", B, 64, 1.0)
        margin = min(margin, float(-ref["terms"][ref["terms"] > 0].log().min()))
        losses, g = R.duo_autograd(a, p, q, 1.0, dtype=torch.float32)
        worst_loss = max(worst_loss, *R.peaked_loss_figures(losses, ref, (1.0, 1.0), B))
        worst_grad = max(worst_grad, R.cancel_figure(g, ref, z, 1.0, (1.0, 1.0), B))
    print(f"peaked: float32 torch loss {worst_loss:.3g}, gradient {worst_grad:.3g}; smallest margin {margin:.3g} nats")
    assert worst_loss <= R.LOSS_TOL / 2 and worst_grad <= R.GRAD_TOL / 2
    assert margin > 3.0                      # every positive wins clearly: the regime where nothing holds relative to itself


def test_workspace_carve_matches_the_header_rule():
    c = R.ws_carve(17)
    assert c["lse"] == (0, 256) and c["term"] == (512, 1024) and c["total"] == 1536
