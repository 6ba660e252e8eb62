"""train8_kernel's policy-tower chain: the head's weights (W_mu rows and W_mu^T) and the action / mask tile that the prologue requests and parks, and wave 0's
column sums of d mu / d logstd and four loss sums behind the d mu tile.  Where in the workgroup these requests, LDS stores and sums sit is a question of speed
(profiles/EXPERIMENTS.md has the placements measured); wherever they sit, no expression changes, so the check is the quantities those pieces feed, at the
smallest shape that still has a live row, a dead row and a dead tile in one launch: a rollout of 8 environments x 5 steps taken as ONE minibatch is one train
step of 40 rows -- two full 16-row tiles, one half-dead tile, and one dead tile behind the host's padding to 64 rows.

Tolerances are tests/test_hip_parity.py's for the same quantities (test_train_step_losses_gradient_and_weights): the mean losses rtol 1e-4 / atol 1e-6, clipfrac
within one row, every gradient entry rtol 2e-4 / atol 2e-6 of the largest entry of the whole reference gradient."""
import numpy as np
import pytest

from oracle import oracle as o
from tests import helpers as H
from tests.masked_categorical_ref import random_masks

pytestmark = pytest.mark.gpu

CR = 0.16102319955825806
LR = 0.000393141177482903
HID = (256, 256)
E, T = 8, 5
N = E * T                                                        # 40 rows = 2 live tiles + 8 live / 8 dead rows + 1 dead tile
# the gradient entries behind those pieces: d b_mu and d logstd are wave 0's column sums; the head's weight gradient is formed from the d mu tile and the
# activations behind the W_mu fragments; the first layer's from x0g and, through d mu W_mu^T, from the transpose's fragments
MOVED = ("pi/b", "pi/logstd", "pi/w", "pi_fc0/w", "vf_fc0/w")


def close(a, b, rtol=1e-4, atol=1e-5, msg=""):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=msg)


def delta(after, before):
    return {k: v - before.get(k, 0) for k, v in after.items() if v != before.get(k, 0)}


def check(losses, ref_losses, grad, ref_grad, block, names):
    """`block(name, vector)`: the tensor's entries of a flat gradient"""
    print("losses", losses, "ref", ref_losses)
    close(losses[:4], ref_losses[:4], rtol=1e-4, atol=1e-6, msg="mean losses")
    assert abs(float(losses[4]) - float(ref_losses[4])) <= 1.01 / N, ("clipfrac", losses[4], ref_losses[4])
    gs = float(np.abs(ref_grad).max())
    for name in names:
        got, want = block(name, grad), block(name, ref_grad)
        assert np.abs(want).max() > 0, name
        print("   %-10s max abs err %.3g (atol %.3g)" % (name, np.abs(got - want).max(), 2e-6 * gs))
        close(got, want, rtol=2e-4, atol=2e-6 * gs, msg="gradient of " + name)
    close(grad, ref_grad, rtol=2e-4, atol=2e-6 * gs, msg="whole gradient")


@pytest.mark.parametrize("O,A", [(18, 18),       # train8_kernel<32, 32>: one action element per lane
                                 (36, 40)])      # train8_kernel<64, 64>: both tiles 64 wide, two action elements per lane (the second live in 8 lanes of a row)
def test_gaussian_one_update_of_40_rows(O, A):
    import ppo_cpp_amd
    orc = o.Oracle(O, A, list(HID))
    orc.init_orthogonal(3)
    orc.tensor("pi/logstd")[:] = np.random.RandomState(4).uniform(-1.0, 0.2, (1, A))
    g = ppo_cpp_amd.PPOHip(O, A, list(HID))
    g.set_flat(orc.theta)
    mb = H.synth_minibatch(orc, N, seed=61)
    args = (mb["obs"], mb["actions"], mb["advs"], mb["returns"], mb["old_neglogp"], mb["old_values"])
    ref_losses, ref_grad = orc.loss_grad(*args, CR)
    k0 = g.kernel_counts()
    losses = g.train_step(LR, CR, *args)
    assert delta(g.kernel_counts(), k0) == {"train8_kernel": 1, "weight_grad_assemble_kernel": 1}
    grad, _ = g.last_grad()
    check(losses, ref_losses, grad, ref_grad, lambda name, vec: orc.tensor(name, vec), MOVED)
    g.close()


def test_masked_categorical_one_update_of_40_rows():
    """every row has a mask of its own (and the first rows are the one-category rows of random_masks): a mask tile parked too late, or in the wrong row, moves the
    normaliser of that row"""
    from tests.test_action_mask import synth_batch
    from tests.test_pair_categorical import make
    O, A = 18, 18
    ref, g = make(O, A, seed=9, ent_coef=0.01)
    mask = random_masks(np.random.RandomState(207), N, A, special=True)
    assert len({m.tobytes() for m in mask}) > N // 2
    batch = synth_batch(ref, N, 107, mask)
    ref_losses, ref_grad = ref.loss_grad(*batch, CR, mask)
    k0 = g.kernel_counts()
    losses = g.train_step(LR, CR, *batch, mask=mask)
    assert delta(g.kernel_counts(), k0) == {"train8_kernel<cat,mask>": 1, "weight_grad_assemble_kernel": 1}
    grad, _ = g.last_grad()
    check(losses, ref_losses, grad, ref_grad, lambda name, vec: ref.t(name, vec), ("pi/b", "pi/w", "pi_fc0/w", "vf_fc0/w"))
    g.close()


def test_multi_binary_one_update_of_40_rows():
    """the bit pattern differs from row to row: an action tile parked too late, or in the wrong row, moves that row's neglogp"""
    from tests.test_multi_binary import synth_batch
    from tests.test_pair_multi_binary import DW2, T8, flagged
    O, A = 18, 24
    ref, g = flagged(O, A, seed=9, ent_coef=0.01)
    batch = synth_batch(ref, N, 108)
    assert len({x.tobytes() for x in batch[1]}) > N // 2
    ref_losses, ref_grad = ref.loss_grad(*batch, CR)
    losses = g.train_step(LR, CR, *batch)
    assert g.kernel_count(T8) == 1 and g.kernel_count(DW2) == 1, g.kernel_variants()
    grad, _ = g.last_grad()
    check(losses, ref_losses, grad, ref_grad, lambda name, vec: ref.t(name, vec), ("pi/b", "pi/w", "pi_fc0/w", "vf_fc0/w"))
    g.close()
