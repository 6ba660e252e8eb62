"""The categorical and multi-categorical heads at trained-policy logits, in every kernel family: one act call and one train step per logit case against the float64
references (tests/categorical_ref.py, tests/masked_categorical_ref.py, tests/multi_categorical_ref.py) at the project's usual tolerances.  Inputs, the fp32
emulation and the fault models are in tests/head_edges_ref.py, where the two parts are described.

CPU tests: the emulation at float64 IS the references' loss and gradient; the inputs are finite, clear of near-ties and of the clip edges; the fp32 emulation passes
every part-1 assertion; five fault models are each rejected by a named case and none by the `mixed` control (the regime every other test of these heads runs in);
the part-2 emulation errors and bounds are printed.
GPU tests (skipped without a device): (family, head form, mask on or off, rows) -> one handle, the logit cases looped inside, then the part-2 case.
    generic   policy_step_kernel / train_fwd_bwd_kernel <cat> <cat,mask> <mcat> <mcat,mask>            hidden (64, 64), rows 1 and 17
    narrow    narrow_step_kernel / narrow_train_kernel, static and runtime shapes                    rows 1 and 33
    host      narrow_host_step: the act call of a one-step rollout behind a host Env (no train step of its own, no deterministic form)   1 and 32 environments
    pair      train8_kernel + weight_grad_assemble_kernel with policy_step_kernel as its act side     hidden (256, 256), 16 rows
    bf16      bf16_step_sequence / bf16_train_sequence                                                 that path's two smallest shapes, 64 rows
The bf16 family: the table is drawn from bf16-representable values and the device's logits ("bf_head_pi") are asserted to EQUAL it.  Its value tower runs on bf16
operands and its d logits are rounded to bf16, so the fp32 tolerances against the fp32-weight references do not apply to the value, vf_loss or the gradient; the
family is held to the derived brackets of tests/test_bf16_categorical.py / tests/test_bf16_multi_categorical.py (their check_act and their check_train, the
latter with an underflow floor, fed the device's own -- here exact -- logits) instead: d logits, the five loss terms and the pi/b gradient; the weights, Adam m and
the global norm after the step are checked for finiteness only (the stage tests own them), plus this file's exact rules (ties, forbidden, single category, finiteness).  It has no part-2 case: tests/test_bf16_stages.py owns that.
"""
import numpy as np
import pytest

from tests import head_edges_ref as E
from tests.categorical_ref import CatRef
from tests.masked_categorical_ref import MaskedCatRef
from tests.multi_categorical_ref import MultiCatRef, offsets

CR, LR = E.CR, E.LR
GAMMA, LAM = 0.99, 0.95
HOST_T = 4
ENT = 0.01


def test_constants_are_the_projects_own():
    from tests import test_discrete_policy as D
    from tests import test_narrow_categorical as N
    assert (E.TIE, E.CR, E.LR) == (D.TIE, D.CR, D.LR) and E.LOGIT_TOL == N.LOGIT_TOL
    from tests import bf16_ref as R
    assert E.PART2_FACTOR == R.RATE_FACTOR == R.L2_FACTOR


# =====================================================================================================================================================
# CPU: the inputs and the comparison's teeth
# =====================================================================================================================================================
CPU_O, CPU_HIDDEN = 18, (64, 64)
CPU_HEADS = {"cat": [18], "mcat": [3, 5, 2, 8]}


def cpu_ref(head, masked):
    nvec = CPU_HEADS[head]
    if head == "mcat":
        return MultiCatRef(CPU_O, nvec, CPU_HIDDEN, ent_coef=ENT)
    return (MaskedCatRef if masked else CatRef)(CPU_O, nvec[0], CPU_HIDDEN, ent_coef=ENT)


def cpu_batches(head, masked, n):
    ref = cpu_ref(head, masked)
    table, forb = E.logit_table(E.nvec_of(ref))
    return ref, forb, [(case, E.exact_batch(ref, CPU_O, table, forb, case, n, masked)) for case in E.cases_for(E.nvec_of(ref))]


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("head", list(CPU_HEADS))
def test_emulation_at_float64_is_the_references_loss_and_gradient(head, masked):
    """emulate() in the references' operand order: at float64 it gives their neglogp, entropy, five loss columns and gradient to 1e-9, on the control, on
    forbidden_high and on the part-2 weights"""
    ref, forb, batches = cpu_batches(head, masked, 17)
    picked = [b for case, b in batches if case in ("mixed", "forbidden_high", "peaked40")] + [E.part2_batch(ref, CPU_O, forb, 17, masked)]
    for b in picked:
        e = E.emulate_batch(ref, b, np.float64)
        ref.theta[:] = b.theta
        losses, grad = E.ref_loss_grad(ref, *b.train_args(), CR, b.mask)
        np.testing.assert_allclose(e["nlp"], b.nlp_train, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(e["ent"], b.ent_rows, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(e["losses"], losses, rtol=1e-9, atol=1e-9)
        np.testing.assert_allclose(e["grad"], grad, rtol=1e-9, atol=1e-9 * np.abs(grad).max())


def test_bf16_table_is_representable_and_keeps_its_shape():
    for nvec in ([2], [128], [2, 62, 64]):
        t32, forb = E.logit_table(nvec)
        t16, forb16 = E.logit_table(nvec, bf16=True)
        np.testing.assert_array_equal(forb, forb16)
        for case, x in t16.items():
            np.testing.assert_array_equal(E.rne_bf16(x), x, err_msg=case)
        assert (np.ptp(t16["high"]) > 0 or len(t16["high"]) == 2) and np.all(np.abs(t16["high"] - 3072) <= 48) and np.all(np.abs(t16["low"] + 200) <= 3)
        assert np.all(t16["forbidden_high"][forb] > 98) and np.all(t16["forbidden_high"][~forb] < -98)


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("head", list(CPU_HEADS))
def test_inputs_are_finite_clear_of_near_ties_and_of_the_clip_edges(head, masked):
    """conditions on the inputs, from the float64 reference alone: every output finite; at least 0.9 of the rows keep their action under a logit perturbation of
    LOGIT_TOL (part 1: the perturbation is zero and every pair is MARGIN clear; part 2 can fall short, and must not); no row within 1e-3 of a clip edge; the edge
    rows are there"""
    seen_single, seen_tiny, seen_one, worst_nlp, worst_share, heavy = False, False, False, 0.0, 0.0, False
    for n in (1, 17, 33):
        ref, forb, batches = cpu_batches(head, masked, n)
        batches.append(("part2", E.part2_batch(ref, CPU_O, forb, n, masked)))
        for case, b in batches:
            want = b.reference_step(ref)
            for x in (b.logits, b.v, b.nlp_train, b.ent_rows, b.pert[np.isfinite(b.pert)], want["losses"], want["grad"], want["theta"], want["m"]):
                assert np.isfinite(x).all(), (case, n)
            gap = E.top2_gap(b.nvec, b.pert)
            clear = (gap > 2 * E.LOGIT_TOL).all(1)
            if case != "part2":
                assert (gap > E.MARGIN).all(), (case, n, gap.min())
            if n > 1:
                assert clear.mean() >= 0.9, (case, n, clear.mean())
            assert E.clip_edge_distance(b.v, b.nlp_train, b.old_nlp, b.old_v) >= 1e-3, (case, n)
            share = E.rounding_share(b, want["grad"])
            worst_share = max(worst_share, share)
            assert share <= 0.5, "%s n=%d: rounding the forced rows' neglogp to float32 alone may use %.2f of the gradient's absolute tolerance" % (case, n, share)
            assert (b.forced.sum() >= 1 or n < 5) and b.forced.sum() <= n // 5 + (n >= 32), (case, n)
            heavy |= bool(n >= 32 and (np.abs(b.adv[b.forced]) > 0.5).any() and b.nlp_train[b.forced][np.abs(b.adv[b.forced]) > 0.5].max() > 1.0)
            if b.mask is not None:
                assert np.all(np.take_along_axis(b.mask, b.train_acts + offsets(b.nvec)[:-1], 1) != 0) and (b.mask.sum(1) >= b.K).all()
                seen_single |= bool(E.single_rows(b.nvec, b.mask).any())
                if case == "forbidden_high":
                    assert np.array_equal(b.mask[0] != 0, ~forb)
            seen_tiny |= bool((b.u == E.TINY).any())
            seen_one |= bool((b.u == E.ONE_M).any())
            if b.forced.any():
                worst_nlp = max(worst_nlp, float(b.nlp_train[b.forced].max()))
    print("largest neglogp of a forced action: %.1f; largest share of the gradient's tolerance that rounding neglogp may use: %.2f" % (worst_nlp, worst_share))
    assert seen_tiny and seen_one and (seen_single or not masked) and worst_nlp > 50.0 and heavy


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("head", list(CPU_HEADS))
def test_fp32_emulation_passes_every_assertion(head, masked):
    for n in (1, 16, 17, 33):
        ref, forb, batches = cpu_batches(head, masked, n)
        for case, b in batches:
            tag = "%s n=%d %s" % (head, n, case)
            E.check_act(b, case, *E.emulated_act(ref, b), tag)
            want = b.reference_step(ref)
            E.check_train(ref, b, E.emulated_train(ref, b), want, tag)
            for seed in range(4):                           # ... and so does a kernel whose neglogp comes out one float32 further up or down, row by row
                E.check_train(ref, b, E.emulated_train(ref, b, nudge=np.random.RandomState(seed)), want, tag + " nudged")
        if masked and n > 1:                                # rows with one allowed category per component: exactly 0 neglogp and entropy
            table, _ = E.logit_table(E.nvec_of(ref))
            b = E.exact_batch(ref, CPU_O, table, forb, "peaked40", 4, True, single=True)
            E.check_act(b, "peaked40", *E.emulated_act(ref, b), "single")
            got = E.emulated_train(ref, b)
            assert got["losses"][2] == 0.0
            E.check_train(ref, b, got, b.reference_step(ref), "single")
        b = E.part2_batch(ref, CPU_O, forb, n, masked)      # the part-2 case under its own bounds
        nlp_x, ent_x, l2, _ = E.part2_bounds(ref, b)
        E.check_act(b, "part2", *E.emulated_act(ref, b), "%s n=%d part2" % (head, n), nlp_extra=nlp_x, margin=2 * E.LOGIT_TOL)
        if n > 1:
            E.check_train(ref, b, E.emulated_train(ref, b, nudge=np.random.RandomState(0)), b.reference_step(ref), "%s n=%d part2" % (head, n), ent_extra=ent_x, grad_l2=l2)


# the case that must reject each fault model (masked rows, 17 of them); `mixed` must reject none.  The control stands for the suite as it was: O(1) logits under the
# rules it had, so its rows with one allowed category are held to |neglogp| <= 1e-6 (tests/test_action_mask.py) where this file asks for exactly 0.
REJECTED_BY = {"max_all": "forbidden_high", "pad0_in_max": "low", "no_max_sub": "high", "act_unchecked": "forbidden_high", "ent_forbidden": "forbidden_high"}


@pytest.mark.parametrize("head", list(CPU_HEADS))
def test_every_fault_model_is_rejected_by_a_named_case_and_none_by_the_control(head):
    ref, forb, batches = cpu_batches(head, True, 17)
    assert set(REJECTED_BY) == set(E.FAULTS)
    for fault in E.FAULTS:
        rejecting = []
        for case, b in batches:
            try:
                E.check_act(b, case, *E.emulated_act(ref, b, fault), case, exact_single=case != "mixed")
                E.check_train(ref, b, E.emulated_train(ref, b, fault), b.reference_step(ref), case)
            except AssertionError:
                rejecting.append(case)
        print("%-14s rejected by %s" % (fault, rejecting))
        assert REJECTED_BY[fault] in rejecting, (fault, rejecting)
        assert "mixed" not in rejecting, "the control alone must not notice %s: that is the gap these tests close" % fault


@pytest.mark.parametrize("head", list(CPU_HEADS))
def test_part2_emulation_errors_and_bounds(head):
    """prints what the fp32 emulation shows against float64 on the part-2 rows and the bounds that follow (recorded in tests/head_edges_ref.py)"""
    key = {"cat": "cat A=18", "mcat": "mcat (3, 5, 2, 8)"}[head]
    worst = np.zeros(3)
    for masked in (False, True):
        ref = cpu_ref(head, masked)
        _, forb = E.logit_table(E.nvec_of(ref))
        b = E.part2_batch(ref, CPU_O, forb, 33, masked)
        nlp_x, ent_x, l2, meas = E.part2_bounds(ref, b)
        print("%s %s: emulation neglogp %.3g entropy %.3g grad rel L2 %.3g -> bounds %.3g / %.3g / %.3g (largest neglogp %.1f)" % (
            key, "masked" if masked else "plain", meas[0], meas[1], meas[2], nlp_x, ent_x, l2, b.nlp_train.max()))
        worst = np.maximum(worst, meas)
        assert np.isfinite([nlp_x, ent_x, l2]).all() and l2 >= 2e-4
    rec = np.array(E.PART2_MEASURED[key])
    assert np.all(worst <= 4.0 * rec) and np.all(rec <= 4.0 * worst), (worst, rec)        # (the BLAS at hand decides the last bits of the fp32 products)


# =====================================================================================================================================================
# GPU
# =====================================================================================================================================================
gpu = pytest.mark.gpu
HEADED = ("policy_step_kernel", "train_fwd_bwd_kernel", "narrow_step_kernel", "narrow_train_kernel", "narrow_host_step", "train8_kernel", "bf16_step_sequence",
          "bf16_train_sequence")


def need_gpu():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def suffix(nvec_or_A, masked):
    return "<%s%s>" % ("cat" if isinstance(nvec_or_A, int) else "mcat", ",mask" if masked else "")


def assert_ran(g, want, allow=()):
    """ppo_kernel_counts: the named kernels ran, and no other step / train kernel of any family or head form did"""
    kc = g.kernel_counts()
    for name in want:
        assert kc[name] > 0, (name, kc)
    for name, cnt in kc.items():
        if name.startswith(HEADED) and name not in want and name not in allow:
            assert cnt == 0, (name, kc)


def bias_word(g, ref):
    """where pi/b[0] lives in the padded parameter vector (the gradient buffer has the same layout)"""
    probe = np.zeros(g.P, np.float32)
    probe[ref.offs["pi/b"][0]] = 7.0
    g.set_flat(probe)
    at = np.nonzero(g.debug_buffer("theta").view(np.float32) == 7.0)[0]
    assert at.size == 1 and at[0] % 256 == 0
    return int(at[0])


def assert_padding_gradient_is_zero(g, at, A, tag):
    """pi/b's padding columns and the logstd slot a discrete handle keeps behind them (one 256-word block each): exactly zero words.  A NaN or a -0.0 is a word."""
    words = g.debug_buffer("grad")
    assert not words[at + A:at + 512].any(), "%s: the gradient of pi/b's padding columns / the logstd slot is not zero" % tag


def reset(g, theta, pw0):
    zero = np.zeros(g.P, np.float32)
    g.set_flat(theta.astype(np.float32))
    g.set_flat(zero, 1)
    g.set_flat(zero, 2)
    g.set_beta_powers(pw0)


def device_train(g, b):
    acts = b.train_acts.astype(np.float32).reshape((b.n,) + g._act_shape)
    losses = g.train_step(LR, CR, b.obs, acts, b.adv, b.ret, b.old_nlp, b.old_v, mask=b.mask)
    grad, norm = g.last_grad()
    return dict(losses=losses, grad=grad, norm=norm, theta=g.get_flat(0), m=g.get_flat(1))


def run_fp32_family(ref, g, O, n, masked, tag, act=None, train=True):
    """every part-1 case and the part-2 case on one handle.  act: the family's act call, b -> (actions, deterministic actions or None, values, neglogp)"""
    nvec = E.nvec_of(ref)
    A = int(sum(nvec))
    table, forb = E.logit_table(nvec)
    pw0 = g.beta_powers()
    at = bias_word(g, ref)
    train = train and n > 1                                 # (ppo_train_step refuses a one-row minibatch, as the reference does: the one-row tests are act calls)
    if act is None:
        def act(b):
            a, v, nlp = g.step(b.obs, b.u, mask=b.mask)
            return a, g.act_deterministic(b.obs, mask=b.mask), v, nlp
    for case in E.cases_for(nvec):
        b = E.exact_batch(ref, O, table, forb, case, n, masked)
        t = "%s %s" % (tag, case)
        reset(g, b.theta, pw0)
        a, det, v, nlp = act(b)
        print("%s: neglogp %s" % (t, np.array2string(np.asarray(nlp)[:4], precision=6)))
        E.check_act(b, case, a, det, v, nlp, t)
        if train:
            got = device_train(g, b)
            print("%s: losses %s" % (t, got["losses"]))
            E.check_train(ref, b, got, b.reference_step(ref), t)
            assert_padding_gradient_is_zero(g, at, A, t)
    if masked:                                              # rows that each allow one category per component: neglogp and entropy exactly 0
        b = E.exact_batch(ref, O, table, forb, "peaked40", 4 if train else n, True, single=True)
        t = tag + " single"
        reset(g, b.theta, pw0)
        a, det, v, nlp = act(b)
        E.check_act(b, "peaked40", a, det, v, nlp, t)
        np.testing.assert_array_equal(nlp, 0.0, err_msg=t)
        if train:
            got = device_train(g, b)
            assert got["losses"][2] == 0.0 and got["losses"][3] > 0.0, (t, got["losses"])
            E.check_train(ref, b, got, b.reference_step(ref), t)
    b = E.part2_batch(ref, O, forb, n, masked)
    nlp_x, ent_x, l2, meas = E.part2_bounds(ref, b)
    t = tag + " part2"
    reset(g, b.theta, pw0)
    a, det, v, nlp = act(b)
    want = E.neglogp_of(nvec, b.logits, np.asarray(a).reshape(n, -1).astype(np.int64), b.mask)
    print("%s: emulation errors %s, neglogp error %.3g (allowance %.3g)" % (t, meas, np.abs(nlp - want).max(), nlp_x))
    E.check_act(b, "part2", a, det, v, nlp, t, nlp_extra=nlp_x, margin=2 * E.LOGIT_TOL)
    if train:
        got = device_train(g, b)
        wantt = b.reference_step(ref)
        print("%s: entropy error %.3g (allowance %.3g), grad rel L2 %.3g (bound %.3g)" % (
            t, abs(got["losses"][2] - wantt["losses"][2]), ent_x, np.linalg.norm(got["grad"] - wantt["grad"]) / np.linalg.norm(wantt["grad"]), l2))
        E.check_train(ref, b, got, wantt, t, ent_extra=ent_x, grad_l2=l2)
        assert_padding_gradient_is_zero(g, at, A, t)


# ---- generic ----------------------------------------------------------------------------------------------------------------------------------------
def make_generic(O, head, hidden, masked, **kw):
    if isinstance(head, int):
        if masked:
            from tests.test_action_mask import make
        else:
            from tests.test_discrete_policy import make
        return make(O, head, hidden, ent_coef=ENT, **kw)
    from tests.test_multi_discrete import make
    return make(O, head, hidden, ent_coef=ENT, **kw)


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("n", [1, 17])
@pytest.mark.parametrize("O,head", [(18, 6), (18, 18), (18, 40), (18, (3, 4)), (36, (2, 2, 2, 2, 20, 3, 33))], ids=["A6", "A18", "A40", "nvec3_4", "nvec_K7_A64"])
def test_generic_kernels(O, head, n, masked):
    need_gpu()
    ref, g = make_generic(O, head, (64, 64), masked)
    s = suffix(head, masked)
    run_fp32_family(ref, g, O, n, masked, "generic" + s)
    assert_ran(g, ["policy_step_kernel" + s] + (["train_fwd_bwd_kernel" + s] if n > 1 else []))
    g.close()


# ---- narrow -----------------------------------------------------------------------------------------------------------------------------------------
def make_narrow(O, head, hidden, **kw):
    if isinstance(head, int):
        from tests.test_narrow_categorical import narrow
    else:
        from tests.test_narrow_multi_discrete import narrow
    return narrow(O, head, hidden, ent_coef=ENT, **kw)


NARROW = [(18, 6, (64, 64)), (36, 18, (64, 64)), (50, 40, (64, 64)), (7, 3, (4, 5)),
          (18, (3, 5, 2, 8), (64, 64)), (36, (2, 2, 2, 2, 20, 3, 33), (64, 64)), (7, (2, 3), (4, 5))]


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("n", [1, 33])
@pytest.mark.parametrize("O,head,hidden", NARROW, ids=["A6", "A18", "A40", "A3_tiny", "nvec3_5_2_8", "nvec_K7_A64", "nvec2_3_tiny"])
def test_narrow_kernels(O, head, hidden, n, masked):
    need_gpu()
    ref, g = make_narrow(O, head, hidden)
    s = suffix(head, masked)
    run_fp32_family(ref, g, O, n, masked, "narrow" + s)
    assert_ran(g, ["narrow_step_kernel" + s] + (["narrow_train_kernel" + s] if n > 1 else []))
    g.close()


# The narrow row's shapes where the fused step takes them: its image (the handle's LDS image plus the step's own state) must fit 160 KB, which behind (64, 64) holds
# for an action tile of 32 columns -- (18, 6), (18, 18), (36, 18), the multi heads -- and not for the 48 columns of (50, 40): that head, and a 64-category one that
# fills all four column slots of a lane, run behind (32, 32) towers as in tests/test_narrow_host_step.py (the head code is the same).  (7, 3) and (7, (2, 3)) behind
# (4, 5) are the runtime-shape instantiation.  Every case asserts that the fused kernel is what ran.  1 and 32 environments (the form takes at most 32).
HOST = [(18, 6, (64, 64)), (18, 18, (64, 64)), (36, 18, (64, 64)), (50, 40, (32, 32)), (18, 64, (32, 32)), (7, 3, (4, 5)),
        (18, (3, 5, 2, 8), (64, 64)), (50, (2, 17, 16, 5), (32, 32)), (7, (2, 3), (4, 5))]


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("n", [1, 32])
@pytest.mark.parametrize("O,head,hidden", HOST, ids=["A6", "A18", "O36_A18", "A40_h32", "A64_h32", "A3_tiny", "nvec3_5_2_8", "nvec2_17_16_5_h32", "nvec2_3_tiny"])
def test_narrow_host_step(O, head, hidden, n, masked):
    """the act call is rollout_act of a rollout of n environments and HOST_T steps with the normaliser off (the smallest rollout tests/test_narrow_host_step.py
    drives); every step is fed the same rows, so every step stores the same actions, values and neglogp, which are what the rollout kept"""
    need_gpu()
    ref, g = make_narrow(O, head, hidden)
    g.set_host_step_fused(True)
    if masked:
        g.set_action_masking(True)
    g.norm_init(n)
    g.rollout_alloc(n, HOST_T)
    g.norm_set_flags(False, False)
    zero = np.zeros(n, np.float32)

    def act(b):
        g.rollout_reset(b.obs)
        acts = []
        for t in range(HOST_T):
            acts.append(g.rollout_act(t, b.u, mask=b.mask))
            g.rollout_observe(t, b.obs, zero, zero)
        g.rollout_finish(GAMMA, LAM)
        got = {f: g.rollout_get(f) for f in ("actions", "values", "neglogp")}
        for t in range(HOST_T):
            np.testing.assert_array_equal(got["actions"][t], acts[0])
            np.testing.assert_array_equal(got["neglogp"][t], got["neglogp"][0])
        return acts[0], None, got["values"][0], got["neglogp"][0]

    run_fp32_family(ref, g, O, n, masked, "host" + suffix(head, masked), act=act, train=False)
    assert_ran(g, ["narrow_host_step" + suffix(head, masked)], allow=["narrow_step_kernel" + suffix(head, False)])      # (rollout_finish's value passes)
    g.close()


# ---- the [256,256] pair -----------------------------------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("O,head", [(36, 18), (50, 64), (18, (3, 5, 2, 8)), (50, (4,) * 16)], ids=["A18", "A64", "nvec3_5_2_8", "nvec_K16_A64"])
def test_pair_kernels(O, head, masked):
    need_gpu()
    if isinstance(head, int):
        from tests.test_pair_categorical import make
    else:
        from tests.test_pair_multi_discrete import make
    ref, g = make(O, head, seed=9, ent_coef=ENT)
    s = suffix(head, masked)
    run_fp32_family(ref, g, O, 16, masked, "pair" + s)
    assert_ran(g, ["policy_step_kernel" + s, "train8_kernel" + s])
    assert g.kernel_counts()["weight_grad_assemble_kernel"] > 0
    g.close()


# ---- bf16 -------------------------------------------------------------------------------------------------------------------------------------------
UNDERFLOW = 2.0 ** -126     # below the smallest normal float32 a term may be flushed to zero or keep only some of its bits: the hardware's choice, not a fault
NORMAL = 2.0 ** -100        # a d logit below this has a factor exp(a0) / z near or under UNDERFLOW: it is held to the bracket, not counted in the rounding share


@gpu
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("hidden,O,head,n", [((128,), 7, 2, 64), ((128,), 7, 128, 64), ((128,), 7, (2, 2), 64), ((128,), 7, (2, 62, 64), 64)],
                         ids=["A2", "A128", "nvec2_2", "nvec2_62_64"])
def test_bf16_sequences(hidden, O, head, n, masked):
    need_gpu()
    if isinstance(head, int):
        from tests import test_bf16_categorical as B
    else:
        from tests import test_bf16_multi_categorical as B
    d = B.Dev(hidden, O, head, ent_coef=ENT)
    ref, g = d.ref, d.g
    nvec = E.nvec_of(ref)
    A = int(sum(nvec))
    table, forb = E.logit_table(nvec, bf16=True)
    pw0 = g.beta_powers()
    at = bias_word(g, ref)
    s = suffix(head, masked)
    for case in E.cases_for(nvec):
        b = E.exact_batch(ref, O, table, forb, case, n, masked)
        t = "bf16%s %s" % (s, case)
        reset(g, b.theta, pw0)
        a, v, nlp = B.check_act(d, b.obs, b.u, b.mask, t)
        lg, _ = d.logits_values(n)
        np.testing.assert_array_equal(lg, np.broadcast_to(table[case], (n, A)), err_msg=t + ": the device's logits are the table, bit for bit")
        assert np.isfinite(a).all() and np.isfinite(v).all() and np.isfinite(nlp).all(), t
        ai = np.asarray(a).reshape(n, -1).astype(np.int64)
        bad = (ai != b.acts) & ~(E.top2_gap(nvec, b.pert) < E.TIE)
        assert not bad.any(), "%s sampled actions: %d pairs differ from the float64 reference" % (t, bad.sum())
        np.testing.assert_array_equal(np.asarray(g.act_deterministic(b.obs, mask=b.mask)).reshape(n, -1), b.det, err_msg=t + " deterministic actions (ties: lowest allowed index)")
        one = E.single_rows(nvec, b.mask)
        if one.any():
            np.testing.assert_array_equal(nlp[one], 0.0, err_msg=t + ": one allowed category")
        want = E.neglogp_of(nvec, b.logits, ai, b.mask)
        assert np.all(np.abs(nlp - want) <= 1e-5 * len(nvec) + 1e-4 * np.abs(want)), (t, np.abs(nlp - want).max())
        # the train step on the reference's actions (forced rows included), around the reference's neglogp of them and the device's own values
        acts = b.train_acts.astype(np.float32).reshape((n,) + g._act_shape)
        _, _, losses, grad = B.check_train(d, b.obs, acts, v, b.nlp_train.astype(np.float32), b.mask, t, seed=300, floor=UNDERFLOW, normal=NORMAL)
        assert np.isfinite(losses).all() and np.isfinite(grad).all() and np.isfinite(g.get_flat(0)).all() and np.isfinite(g.get_flat(1)).all(), t
        lg, _ = d.logits_values(n)
        np.testing.assert_array_equal(lg, np.broadcast_to(table[case], (n, A)), err_msg=t + ": the train pass's logits are the table, bit for bit")
        for name, _ in ref.specs:
            if name.startswith("pi_fc"):
                x = ref.t(name, grad)
                np.testing.assert_array_equal(x, np.zeros(x.shape), err_msg="%s: pi/w = 0, so the gradient of %s is exactly zero" % (t, name))
        if b.mask is not None:
            dead = np.all(b.mask == 0, axis=0)
            np.testing.assert_array_equal(ref.t("pi/b", grad)[dead], 0.0)
            np.testing.assert_array_equal(ref.t("pi/w", grad)[:, dead], 0.0)
        assert_padding_gradient_is_zero(g, at, A, t)
    assert_ran(g, ["bf16_step_sequence" + s, "bf16_train_sequence" + s])
    d.close()
