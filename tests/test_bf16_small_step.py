"""The small-batch forward of a PPO_BF16 handle (ppo_set_bf16_small_step: bf16_small_forward_kernel<RT>; include/ppo_hip.h): at 64 rows or fewer the hidden layers run as
16-row MFMA tiles with the columns split over the workgroups instead of 128-row tile GEMMs.  The claim is BIT identity with the tile path on every live row, under
every head form, so the tests compare a flagged handle with an unflagged one on the same weights with np.array_equal; the kernel's own outputs are also held to float64
by tests/bf16_ref.py's hidden-layer stage under the criterion tests/test_bf16_stages.py applies to the tile GEMM (check_bf16: derived bracket, mismatch share against
the CPU fp32 emulation's).  gauss: unequal widths, Kp0 = 128, K = 384; cat / wcat: the narrow and the wide categorical head behind the kernel.  Rows 1, 16, 17 (RT = 2,
fifteen staged zero rows), 64 (RT = 4, the limit)."""
import numpy as np
import pytest

from tests import bf16_ref as R

pytestmark = pytest.mark.gpu
O, NAME = 20, "bf16_small_forward"
HANDLES = {"gauss": ((256, 128, 384), 6, {}), "cat": ((128, 256), 10, dict(action_dist="categorical", bf16_head=True)),
           "wcat": ((256, 256), 200, dict(action_dist="categorical", bf16_head=True, bf16_wide_head=True))}
same = np.testing.assert_array_equal


def pair(kind, dtype=1):
    """(unflagged handle, flagged handle) with the same weights: orthogonal / random init with the head gain raised so that the head outputs are not all near zero"""
    import ppo_cpp_amd
    from oracle import oracle as o
    from tests.masked_categorical_ref import MaskedCatRef
    hidden, A, kw = HANDLES[kind]
    if kind == "gauss":
        ref = o.Oracle(O, A, list(hidden)); ref.init_orthogonal(7); ref.tensor("pi/w")[:] *= np.float32(2.0 / 0.01)
    else:
        ref = MaskedCatRef(O, A, hidden); ref.init_random(9, 1.0)
    gs = [ppo_cpp_amd.PPOHip(O, A, list(hidden), compute_dtype=dtype, **kw) for _ in range(2)]
    for g in gs:
        g.set_flat(np.asarray(ref.theta, np.float32)); g.seed(5)
    gs[1].set_bf16_small_step(True)
    assert gs[1].bf16_small_step is True and gs[0].bf16_small_step is False
    return gs


def inputs(kind, n):
    rng, A = np.random.RandomState(100 + n), HANDLES[kind][1]
    noise = rng.normal(size=(n, A)) if kind == "gauss" else np.clip(rng.uniform(size=(n, A)), 1e-6, 1 - 1e-6)
    return rng.uniform(-2, 2, (n, O)).astype(np.float32), noise.astype(np.float32)


@pytest.mark.parametrize("n", [1, 16, 17, 64])
@pytest.mark.parametrize("kind", list(HANDLES))
def test_same_bits_as_the_tile_path(kind, n):
    (g0, g1), (obs, noise) = pair(kind), inputs(kind, n)
    for call in (lambda g: g.step(obs, noise), lambda g: g.step(obs), lambda g: g.act_deterministic(obs), lambda g: g.value(obs)):
        before = g1.kernel_count(NAME)
        for x, y in zip(_tuple(call(g0)), _tuple(call(g1))):
            same(x, y)
        assert g1.kernel_count(NAME) == before + 1, "one count per call that took the small form"
    assert g0.kernel_count(NAME) == 0
    assert np.abs(g1.value(obs)).max() > 0


def _tuple(x):
    return x if isinstance(x, tuple) else (x,)


def test_float64_reference_of_every_layer():
    """n = 17: the kernel's live rows (RT = 2: 32 of them, 15 from staged zero rows) against float64 on the stage's OWN device input, rounding included"""
    hidden, A, _ = HANDLES["gauss"]
    g, n, rows = pair("gauss")[1], 17, 32
    g.value(inputs("gauss", n)[0])
    lay = R.Layout(O, A, hidden)
    th = g.debug_buffer("theta").view(np.float32)
    mir = R.from_bits(g.debug_buffer("bf_theta").view(np.uint16))
    pf, pw = lay.params(th), lay.params(mir)
    bf = lambda name, width: R.from_bits(g.debug_buffer(name).view(np.uint16)).reshape(-1, width)[:rows]
    x0 = bf("bf_x0", lay.Kp0)
    assert x0[:n].any() and not x0[n:].any()
    for t, tw in enumerate(("pi", "vf")):
        x = x0
        for l in range(lay.L):
            q = bf("bf_h_%s_%d" % (tw, l), lay.Hp[l])
            y, E = R.hidden_forward(x, pw["W"][t][l], pf["b"][t][l])
            share_ref = R.mismatch_share(R.emu_hidden_forward(x, pw["W"][t][l], pf["b"][t][l]), y)
            R.check_bf16("small forward %s layer %d" % (tw, l), q, y, E, share_ref)
            assert np.abs(q[:n, :hidden[l]]).min() > 0, "every live element was written"
            x = q


def test_scope_more_rows_the_train_step_collect_synthetic_and_fp32_handles_keep_their_kernels():
    g0, g1 = pair("gauss")
    obs, noise = inputs("gauss", 65)
    outs = []
    for g in (g0, g1):
        a, v, nlp = g.step(obs, noise)
        m = 33
        losses = g.train_step(3e-4, 0.2, obs[:m], a[:m], np.linspace(-1, 1, m).astype(np.float32), v[:m] + 0.1, nlp[:m], v[:m])
        g.rollout_alloc(5, 3); g.collect_synthetic(3, 0.99, 0.95)                      # 5 environments: its per-step launches and value pass keep the tile GEMMs
        outs.append((a, v, nlp, np.asarray(losses), g.get_flat(), g.rollout_get("values"), g.rollout_get("neglogp"), g.rollout_get("returns")))
    for x, y in zip(*outs):
        same(x, y)
    assert g1.kernel_count(NAME) == 0
    f0, f1 = pair("gauss", dtype=0)
    same(f0.value(obs[:8]), f1.value(obs[:8]))
    assert f1.kernel_variants()[NAME] == 0 and f1.kernel_counts() == f0.kernel_counts()


def test_host_env_rollout_matches_the_tile_path():
    from oracle import oracle as o
    E, T, fields = 5, 3, []
    for g in pair("gauss"):
        g.norm_init(E); g.rollout_alloc(E, T)
        g.rollout_reset(o.seeded_env_step(99, 0, E, 0, O)[0])
        g.seed(21)
        for t in range(T):
            g.rollout_act(t)
            g.rollout_observe(t, *o.seeded_env_step(99, 0, E, t + 1, O))
        g.rollout_finish(0.99, 0.95)
        fields.append([g.rollout_get(f) for f in ("actions", "values", "neglogp", "returns")] + [g.kernel_count(NAME)])
    for x, y in zip(fields[0][:4], fields[1][:4]):
        same(x, y)
    assert fields[0][4] == 0 and fields[1][4] >= T
