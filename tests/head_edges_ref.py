"""Inputs, fp32 emulation and fault models for tests/test_head_edges.py: the categorical and multi-categorical heads at trained-policy logits.

Every other test of the discrete heads feeds logits within a few units of zero, where softmax's shift invariance hides a maximum taken over the wrong set, a
padding column in the maximum, a dropped max subtraction, and a 0 * large product.  Here the logits are spread by tens to thousands.

Part 1, exact logits.  pi/w = 0 and pi/b = a row of logit_table(): the logits of every row ARE the bias, bit for bit, on the device and in the references, so the
project's usual tolerances apply unchanged.  Rows differ in mask, action and uniform draw (edge_masks, edge_uniforms, train_actions).
Part 2, row-dependent logits.  init_random(seed, pi_gain=40) and a pi/b that lifts the forbidden block 100 above the allowed one (part2_theta).  Matmul rounding
enters, so the bound is PART2_FACTOR x what emulate(.., np.float32) shows against float64, never tighter than the usual tolerances (part2_bounds).

No second reference: every expected value comes from tests/categorical_ref.py, tests/masked_categorical_ref.py and tests/multi_categorical_ref.py (their float64
softmax_stats / masked_softmax_stats / (masked_)gumbel_argmax and their torch-float64 loss_grad).  emulate() is NOT a reference: it is the same forward, loss and
backward written out in NumPy at a chosen dtype, in the references' operand order.  At float64 it must reproduce loss_grad to 1e-9 (checked on the CPU); at float32
it is the stand-in for a correct kernel (it must pass every part-1 assertion) and, with fault=.., for a subtly wrong one (each must be rejected by a named case,
none by the `mixed` control).

MEASURED part-2 emulation errors (fp32 NumPy against float64 at O = 18, hidden (64, 64), 33 rows, the larger of masked and plain;
tests/test_head_edges.py::test_part2_emulation_errors_and_bounds prints them and holds PART2_MEASURED below to them) and the bounds that follow, 10 x them, used
beside the usual tolerances (neglogp 1e-5 K + 1e-4 |x|, entropy 1e-6 K + 1e-4 |x|) and never below the gradient's usual 2e-4:
                          neglogp (largest |error| over the allowed categories)   entropy (minibatch mean)     gradient (relative L2)
    cat, A = 18           2.0e-5 -> allowance 2.0e-4                              1.7e-8 -> allowance 1.7e-7   7.4e-6 -> bound 2e-4 (the floor)
    mcat, (3, 5, 2, 8)    2.2e-5 -> allowance 2.2e-4                              5.3e-8 -> allowance 5.3e-7   3.8e-6 -> bound 2e-4 (the floor)
The GPU tests compute the three figures for their own shape and rows in the same way (part2_bounds); on an MI355X every family stayed below 1.5e-5 in neglogp
(of the chosen action), 1.2e-6 in entropy (inside the usual tolerance) and 8e-6 in the gradient's relative L2 error.

Part 1's tolerances and a correct kernel: a neglogp of 200 is known to half a float32 ulp (7.6e-6) at best, which reaches the gradient times |adv| / n.  That is
why the forced actions sit on the rows with the smallest advantages and in one component per row (train_actions), why a one-row minibatch is an act-only case (the
library refuses to train on one row anyway), and why the CPU tests also push every row's neglogp one ulp up or down before they ask the emulation to pass.
"""
import numpy as np

from tests.categorical_ref import CatRef, gumbel_argmax, softmax_stats
from tests.masked_categorical_ref import MaskedCatRef, masked_gumbel_argmax, masked_softmax_stats
from tests.masked_categorical_ref import random_masks as cat_random_masks
from tests.multi_categorical_ref import MultiCatRef, offsets
from tests.multi_categorical_ref import random_masks as multi_random_masks

CR = 0.16102319955825806
LR = 0.000393141177482903
TIE = 1e-5              # tests/test_discrete_policy.TIE: a (row, component) whose two best (perturbed) logits are closer than this may go either way in fp32
LOGIT_TOL = 1e-4        # tests/test_narrow_categorical.LOGIT_TOL: two fp32 evaluations of the same logits agree to this
PART2_FACTOR = 10.0     # tests/bf16_ref.RATE_FACTOR / L2_FACTOR: the allowance over what the CPU fp32 emulation shows
TINY = np.float32(2.0 ** -126)          # the smallest positive normal float32: -log(-log u) = -4.47
ONE_M = np.float32(1.0 - 2.0 ** -24)    # the largest float32 below 1:          -log(-log u) = +16.6
MARGIN = 1e-3           # part 1: every (row, component)'s two best perturbed logits are further apart than this (edge_uniforms redraws until they are); the fp32
#                         evaluation of l - log(-log u) at |l| = 3075 is good to 2 x 2^-24 x 3100 = 3.7e-4 (tests/bf16_cat_ref.py, E_pl)

CASES = ("peaked40", "peaked120", "low", "high", "forbidden_high", "ties", "two_ties", "mixed")
MULTI_CASE = "fh_beside_ties"           # multi-categorical only: component 0 forbidden_high, component 1 ties, the rest mixed
FAULTS = ("max_all", "pad0_in_max", "no_max_sub", "act_unchecked", "ent_forbidden")

# test_part2_emulation_errors_and_bounds: (neglogp max abs error, entropy abs error of the mean, gradient relative L2 error) of emulate(float32) against float64 at
# O = 18, hidden (64, 64), 33 rows, masked / unmasked -- the largest over both
PART2_MEASURED = {
    "cat A=18": (2.0e-5, 1.7e-8, 7.4e-6),             # -> allowances 2.0e-4 / 1.7e-7 beside the usual tolerances, gradient bound 2e-4 (the floor)
    "mcat (3, 5, 2, 8)": (2.2e-5, 5.3e-8, 3.8e-6),    # -> 2.2e-4 / 5.3e-7, gradient bound 2e-4 (the floor)
}


def cases_for(nvec):
    return CASES + ((MULTI_CASE,) if len(nvec) > 1 else ())


def nvec_of(ref):
    return list(ref.nvec) if isinstance(ref, MultiCatRef) else [ref.A]


def rne_bf16(x):
    from tests import bf16_ref as R
    return R.rne_bf16(np.asarray(x, np.float32)).astype(np.float32)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------------------------
def two_tie_indices(nk):
    """indices 2 and 16 where the component is wider than 16 (two lanes' different slots), else two distinct ones of its own"""
    if nk > 16:
        return 2, 16
    return (nk // 3 if nk > 2 else 0), nk - 1


def logit_table(nvec, bf16=False):
    """{case: float32 [A]} and the forbidden pattern [A] (bool) that forbidden_high is written for: at least one forbidden and one allowed category per component.
    bf16: every entry is a bf16-representable value (3072 +- 3 would all round to 3072, so `high` takes steps of 16, the bf16 spacing there)."""
    rng = np.random.RandomState(20261020)
    off = offsets(nvec)
    A = int(off[-1])
    forb = np.zeros(A, bool)
    t = {c: np.zeros(A, np.float64) for c in CASES + (MULTI_CASE,)}
    for k, nk in enumerate(nvec):
        s = slice(int(off[k]), int(off[k + 1]))
        f = rng.uniform(size=nk) < 0.5
        keep, drop = rng.permutation(nk)[:2]
        f[keep], f[drop] = False, True
        forb[s] = f
        noise = {c: rng.uniform(-1, 1, nk) for c in CASES}
        t["peaked40"][s] = 40.0 * noise["peaked40"]
        t["peaked120"][s] = 120.0 * noise["peaked120"]
        t["low"][s] = np.round(-200.0 + 3.0 * noise["low"]) if bf16 else -200.0 + 3.0 * noise["low"]
        t["high"][s] = 3072.0 + (16.0 * np.round(3.0 * noise["high"]) if bf16 else 3.0 * noise["high"])
        t["forbidden_high"][s] = np.where(f, 100.0, -100.0) + noise["forbidden_high"]
        t["ties"][s] = 1.5
        t["two_ties"][s] = -5.0
        i, j = two_tie_indices(nk)
        t["two_ties"][s][[i, j]] = 5.0
        t["mixed"][s] = 2.0 * noise["mixed"]
        t[MULTI_CASE][s] = t["forbidden_high"][s] if k == 0 else t["ties"][s] if k == 1 else t["mixed"][s]
    out = {c: (rne_bf16(x) if bf16 else x.astype(np.float32)) for c, x in t.items()}
    return out, forb


def exact_theta(ref, seed, bias):
    """init_random(seed) for the towers and the value head, pi/w = 0, pi/b = bias: every row's logits equal `bias` bit for bit"""
    ref.init_random(seed)
    ref.t("pi/w")[:] = 0.0
    ref.t("pi/b")[:] = np.asarray(bias, np.float64)
    return ref.theta.copy()


def part2_theta(ref, seed, forb):
    """init_random(seed, pi_gain=40) with the forbidden block's bias 100 above the allowed one: logits differ per row and lane"""
    ref.init_random(seed, 40.0)
    ref.t("pi/b")[:] += np.where(forb, 100.0, 0.0)
    ref.theta[:] = ref.theta.astype(np.float32)
    return ref.theta.copy()


def _repair(mask, nvec, prefer):
    """every (row, component) keeps one allowed category: where none is left, the first one of `prefer` [A] (bool) inside the component"""
    off = offsets(nvec)
    for k in range(len(nvec)):
        s = slice(int(off[k]), int(off[k + 1]))
        empty = mask[:, s].sum(1) == 0
        mask[empty, int(off[k]) + int(np.argmax(prefer[s]))] = 1.0
    return mask


def edge_masks(rng, nvec, n, bias, forb, case_index, fh):
    """[n, A] float32.  random_masks(special=True) of the head's own reference file (its first rows: only the first / only the last category, (only those >= 16,)
    all allowed), then four more rows: the complement of `forb`, only the lowest-logit category of every component, only the columns of the last (partly padded)
    16-lane group -- a component without one keeps its last category --, all allowed.  The rows are rotated by the case's index, so that a one-row test meets a
    different one per case.  fh (forbidden_high): every odd row allows only categories outside `forb`, and row 0 is the complement itself."""
    off = offsets(nvec)
    A, K = int(off[-1]), len(nvec)
    m = max(n, 8)
    mask = cat_random_masks(rng, m, A, special=True) if K == 1 else multi_random_masks(rng, m, nvec, special=True)
    comp = (~forb).astype(np.float32)
    lowest, last = np.zeros(A, np.float32), np.zeros(A, np.float32)
    g0 = 16 * ((A - 1) // 16)
    for k in range(K):
        s = slice(int(off[k]), int(off[k + 1]))
        lowest[int(off[k]) + int(np.argmin(bias[s]))] = 1.0
        cols = np.arange(int(off[k]), int(off[k + 1]))
        if (cols >= g0).any():
            last[cols[cols >= g0]] = 1.0
        else:
            last[cols[-1]] = 1.0
    mask[4:8] = [comp, lowest, last, np.ones(A, np.float32)]
    if fh:
        mask[1::2] *= comp
        _repair(mask, nvec, ~forb)
    mask = np.roll(mask, -(case_index % 8), axis=0)
    if fh:
        mask[0] = comp
    return np.ascontiguousarray(mask[:n])


def top2_gap(nvec, x):
    """[n, K]: distance of the two best entries of every component of x [n, A] (-inf = forbidden; a component with one allowed category: inf)"""
    off = offsets(nvec)
    gaps = []
    for k in range(len(nvec)):
        xs = x[:, int(off[k]):int(off[k + 1])]
        if xs.shape[1] == 1:
            gaps.append(np.full(len(x), np.inf))
            continue
        s = np.sort(xs, axis=1)[:, -2:]
        with np.errstate(invalid="ignore"):
            gaps.append(np.where(np.isinf(s[:, 0]), np.inf, s[:, 1] - s[:, 0]))
    return np.stack(gaps, axis=1)


def perturbed(logits, u, mask):
    with np.errstate(divide="ignore"):
        pert = np.asarray(logits, np.float64) - np.log(-np.log(np.asarray(u, np.float64)))
    return pert if mask is None else np.where(mask != 0, pert, -np.inf)


def edge_uniforms(rng, nvec, n, logits, mask, case_index, margin=MARGIN):
    """[n, A] float32 uniforms in [TINY, ONE_M].  Row i holds TINY in lane i % A where (i + case_index) % 6 == 3 and ONE_M there where it is 5 (both keep the
    Gumbel term finite).  Rows whose two best perturbed allowed logits are within `margin` in some component are redrawn: a condition on the inputs."""
    A = int(sum(nvec))

    def draw(rows):
        u = np.clip(rng.uniform(size=(len(rows), A)).astype(np.float32), TINY, ONE_M)
        for r, i in enumerate(rows):
            if (i + case_index) % 6 == 3:
                u[r, i % A] = TINY
            if (i + case_index) % 6 == 5:
                u[r, i % A] = ONE_M
        return u

    u = draw(np.arange(n))
    lg = np.broadcast_to(np.asarray(logits, np.float64), (n, A))
    for _ in range(200):
        close_rows = np.nonzero((top2_gap(nvec, perturbed(lg, u, mask)) <= margin).any(1))[0]
        if close_rows.size == 0:
            return u
        u[close_rows] = draw(close_rows)
    raise AssertionError("edge_uniforms: rows %s stay within %g" % (close_rows, margin))


# ---- the references' own functions, per component ------------------------------------------------------------------------------------------------------------
def head_stats(nvec, logits, mask=None):
    """per component: (neglogp of every category, entropy, probabilities) by softmax_stats / masked_softmax_stats"""
    off = offsets(nvec)
    out = []
    for k in range(len(nvec)):
        s = slice(int(off[k]), int(off[k + 1]))
        out.append(softmax_stats(logits[:, s]) if mask is None else masked_softmax_stats(logits[:, s], mask[:, s]))
    return out


def neglogp_of(nvec, logits, acts, mask=None):
    """row totals of the components' neglogp of acts [n, K], added in component order (MultiCatRef.neglogp_of)"""
    acts = np.asarray(acts).astype(np.int64).reshape(len(logits), len(nvec))
    tot = None
    for k, (nlp_all, _, _) in enumerate(head_stats(nvec, logits, mask)):
        x = nlp_all[np.arange(len(acts)), acts[:, k]]
        tot = x if tot is None else tot + x
    return tot


def entropy_of(nvec, logits, mask=None):
    tot = None
    for _, ent, _ in head_stats(nvec, logits, mask):
        tot = ent if tot is None else tot + ent
    return tot


def sample_actions(nvec, logits, u, mask=None):
    """(actions [n, K], perturbed logits [n, A] with -inf on forbidden ones) by gumbel_argmax / masked_gumbel_argmax per component"""
    off = offsets(nvec)
    acts, perts = [], []
    for k in range(len(nvec)):
        s = slice(int(off[k]), int(off[k + 1]))
        a, p = gumbel_argmax(logits[:, s], u[:, s]) if mask is None else masked_gumbel_argmax(logits[:, s], u[:, s], mask[:, s])
        acts.append(a); perts.append(p)
    return np.stack(acts, 1), np.concatenate(perts, 1)


def det_actions(nvec, logits, mask=None):
    """argmax over the allowed set per component, lowest index on a tie (np.argmax, like tf.argmax: the rule ppo_head.hpp documents)"""
    off = offsets(nvec)
    x = logits if mask is None else np.where(mask != 0, logits, -np.inf)
    return np.stack([np.argmax(x[:, int(off[k]):int(off[k + 1])], axis=1) for k in range(len(nvec))], 1)


FORCED_ADV = 0.1
HEAVY_BUDGET = 1e-8     # what rounding the heavy forced row's neglogp may move a gradient element by: a tenth of the smallest absolute tolerance met (2e-6 x 0.05)


def train_actions(nvec, logits, u, mask, adv):
    """the reference's own Gumbel argmax; on up to a fifth of the rows the least likely allowed category instead, in ONE component (row i: component i % K).
    Which rows, and why one component: a neglogp of 200 is known to half a float32 ulp, 7.6e-6, at best, and a row passes that on to the gradient times |adv| / n.
    With 16 or 17 rows and the gradient's absolute tolerance of 2e-6 of its largest element (about 0.1 here: the value tower's), a row with |adv| = 1 uses the
    tolerance up by rounding alone, whichever way a correct kernel rounds.  So the forced rows are the n // 5 with the smallest |adv| (the advantages do not depend
    on the actions), and beyond the first of those only the ones with |adv| <= FORCED_ADV: three such rows among 17 can move an element by 3 x 7.6e-6 x 0.1 / 17 = 1.3e-7 at most.
    Those rows enter the gradient with a weight of 0.1 / n at most, so a fault in their a0 read shows in neglogp, approxkl and pg_loss more than in the gradient.
    With 32 rows or more one further row is forced, the one whose |adv| is nearest 1 (full weight in the gradient): it takes the least likely allowed category
    whose neglogp keeps half an ulp x |adv| / n inside HEAVY_BUDGET (a neglogp below 8 at 33 rows), or stays as sampled where no category does.
    Four components forced at once (neglogp 800, an ulp of 6e-5 in old_neglogp itself) are not asked for.  rounding_share() states the condition; the CPU tests
    check it on every case, and that a kernel whose neglogp rounds the other way on every row still passes (emulate's nudge)."""
    acts, _ = sample_actions(nvec, logits, u, mask)
    n = len(logits)
    rows = np.arange(n)
    forced = np.zeros(n, bool)
    order = np.argsort(np.abs(adv), kind="stable")[:n // 5]
    forced[order] = True
    forced &= np.abs(adv) <= FORCED_ADV
    forced[order[:1]] = True                                 # (the row with the smallest |adv| in any case: every case of five rows or more has a forced row)
    heavy = int(np.argmin(np.abs(np.abs(adv) - 1.0))) if n >= 32 else -1
    for k, (nlp_all, _, _) in enumerate(head_stats(nvec, logits, mask)):
        worst = np.argmax(np.where(np.isinf(nlp_all), -np.inf, nlp_all), axis=1)
        here = forced & (rows % len(nvec) == k)
        acts[here, k] = worst[here]
        if heavy >= 0 and heavy % len(nvec) == k and not forced[heavy]:
            # one row that enters the gradient with full weight (|adv| nearest 1): the least likely allowed category whose neglogp the budget still allows
            cand = nlp_all[heavy]
            fits = np.isfinite(cand) & (np.spacing(np.abs(cand).astype(np.float32)).astype(np.float64) / 2 * abs(adv[heavy]) / n <= HEAVY_BUDGET)
            if fits.any():
                acts[heavy, k] = int(np.argmax(np.where(fits, cand, -np.inf)))
    if heavy >= 0:
        forced[heavy] = True
    return acts, forced


def rounding_share(b, grad):
    """what half-ulp roundings of the FORCED rows' float32 neglogp can move a gradient element by at most (sum over those rows of ulp/2 |adv| / n: |h| <= 1,
    |p - onehot| <= 1, ratio about 1), as a share of the gradient's absolute tolerance 2e-6 max|grad|"""
    half_ulp = np.spacing(np.abs(b.nlp_train[b.forced]).astype(np.float32)).astype(np.float64) / 2
    return float((half_ulp * np.abs(b.adv[b.forced])).sum() / b.n / (2e-6 * np.abs(grad).max()))


def synth_from(v, nlp, seed, cr=CR):
    """tests/test_discrete_policy.synth_batch's recipe around given reference outputs: (advs, returns, old_neglogp, old_values), rows 1e-3 clear of the clip edges.
    One row (CPU tests only: the library trains on two rows or more) cannot be normalised (its advantage would be 0) and must not sit in a clipped branch (its whole gradient would be 0, and nothing would set the
    gradient's scale): it gets fixed offsets inside both clip ranges and keeps returns - old_values as its advantage."""
    rng = np.random.RandomState(seed)
    n = len(v)
    if n == 1:
        old_nlp, old_v, ret = (nlp + 0.05).astype(np.float32), (v - 0.05).astype(np.float32), (v + 0.5).astype(np.float32)
        return (ret - old_v).astype(np.float32), ret, old_nlp, old_v
    old_nlp = (nlp + rng.normal(scale=0.15, size=n)).astype(np.float32)
    old_v = (v + rng.normal(scale=0.2, size=n)).astype(np.float32)
    ret = (v + rng.normal(scale=0.5, size=n)).astype(np.float32)
    ratio = np.exp(old_nlp.astype(np.float64) - nlp)
    near = np.abs(np.abs(ratio - 1.0) - cr) < 1e-3
    old_nlp[near] += np.float32(0.01)
    dvo = v - old_v
    near = np.abs(np.abs(dvo) - cr) < 1e-3
    old_v[near] -= np.float32(0.01) * np.sign(dvo[near]).astype(np.float32)
    dvo = v - old_v
    vclip = old_v + np.clip(dvo, -cr, cr)
    s1, s2 = (v - ret) ** 2, (vclip - ret) ** 2
    near = (np.abs(dvo) > cr) & (np.abs(s1 - s2) < 1e-3 * np.maximum(s1, 1e-6))
    ret[near] += np.float32(0.05)
    adv = ret - old_v
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    return adv.astype(np.float32), ret, old_nlp, old_v


def clip_edge_distance(v, nlp, old_nlp, old_v, cr=CR):
    """smallest distance of a row to the ratio's and the value's clip edges"""
    ratio = np.exp(np.asarray(old_nlp, np.float64) - nlp)
    return float(min(np.abs(np.abs(ratio - 1.0) - cr).min(), np.abs(np.abs(v - np.asarray(old_v, np.float64)) - cr).min()))


def ref_loss_grad(ref, obs, acts, adv, ret, old_nlp, old_v, cr, mask):
    """the reference's torch-float64 loss_grad, whichever of the three classes `ref` is (acts [n, K])"""
    if isinstance(ref, MultiCatRef):
        return ref.loss_grad(obs, acts, adv, ret, old_nlp, old_v, cr, mask)
    if isinstance(ref, MaskedCatRef):
        return ref.loss_grad(obs, acts[:, 0], adv, ret, old_nlp, old_v, cr, mask)
    assert mask is None
    return ref.loss_grad(obs, acts[:, 0], adv, ret, old_nlp, old_v, cr)


def adam_after(ref, theta0, grad, lr=LR):
    """one clip_by_global_norm + Adam step of the reference from theta0 with fresh slots and beta powers: (theta, m, global norm)"""
    ref.theta[:] = theta0
    ref.m[:] = 0.0
    ref.v[:] = 0.0
    ref.pow = [ref.b1, ref.b2]
    with np.errstate(invalid="ignore", divide="ignore"):
        norm = ref.clip_adam(np.asarray(grad, np.float64), lr)
    out = ref.theta.copy(), ref.m.copy(), norm
    ref.theta[:] = theta0
    return out


class Batch:
    """one case's rows: everything the device and the reference are fed, and what the float64 reference makes of it"""

    def __init__(self, ref, theta, obs, u, mask, seed):
        self.nvec = nvec_of(ref)
        self.K, self.n = len(self.nvec), len(obs)
        self.theta, self.obs, self.u, self.mask = theta, obs, u, mask
        ref.theta[:] = theta
        self.logits, self.v = ref.forward(obs)
        self.acts, self.pert = sample_actions(self.nvec, self.logits, u, mask)
        self.det = det_actions(self.nvec, self.logits, mask)
        adv0 = synth_from(self.v, np.zeros(self.n), seed)[0]              # (the advantages come from the values alone)
        self.train_acts, self.forced = train_actions(self.nvec, self.logits, u, mask, adv0)
        self.nlp_train = neglogp_of(self.nvec, self.logits, self.train_acts, mask)
        self.adv, self.ret, self.old_nlp, self.old_v = synth_from(self.v, self.nlp_train, seed)
        assert np.array_equal(self.adv, adv0)
        self.ent_rows = entropy_of(self.nvec, self.logits, mask)

    def train_args(self):
        return self.obs, self.train_acts.astype(np.float32), self.adv, self.ret, self.old_nlp, self.old_v

    def reference_step(self, ref):
        """(losses, gradient, theta, Adam m, global norm) of one train step of the float64 reference from self.theta"""
        ref.theta[:] = self.theta
        losses, grad = ref_loss_grad(ref, *self.train_args(), CR, self.mask)
        theta, m, norm = adam_after(ref, self.theta, grad)
        return dict(losses=losses, grad=grad, theta=theta, m=m, norm=norm)


def exact_batch(ref, O, table, forb, case, n, masked, seed=5, single=False):
    """the rows of one part-1 case.  single: every row's mask leaves ONE category per component (the first one, the lowest-logit one, the last one, in turn)"""
    nvec = nvec_of(ref)
    ci = cases_for(nvec).index(case)
    rng = np.random.RandomState(1000 + 37 * ci + n)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    bias = table[case]
    fh = case in ("forbidden_high", MULTI_CASE)
    mask = edge_masks(rng, nvec, n, bias, forb, ci, fh) if masked else None
    if single:
        pats = edge_masks(np.random.RandomState(0), nvec, 8, bias, forb, 0, False)[[0, 5, 1]]
        mask = np.ascontiguousarray(pats[np.arange(n) % 3])
        assert single_rows(nvec, mask).all()
    u = edge_uniforms(rng, nvec, n, bias, mask, ci)
    theta = exact_theta(ref, seed, bias)
    return Batch(ref, theta, obs, u, mask, 300 + ci)


def part2_batch(ref, O, forb, n, masked, seed=6):
    """the rows of the part-2 case: under a mask, every row forbids the lifted block (and, at random, half of the rest)"""
    nvec = nvec_of(ref)
    rng = np.random.RandomState(4000 + n)
    obs = rng.uniform(-1, 1, (n, O)).astype(np.float32)
    mask = None
    if masked:
        A = int(sum(nvec))
        mask = cat_random_masks(rng, n, A, special=False) if len(nvec) == 1 else multi_random_masks(rng, n, nvec, special=False)
        mask = _repair(mask * (~forb).astype(np.float32), nvec, ~forb)
    u = np.clip(rng.uniform(size=(n, int(sum(nvec)))).astype(np.float32), TINY, ONE_M)
    theta = part2_theta(ref, seed, forb)
    return Batch(ref, theta, obs, u, mask, 77)


# ---- the same forward, loss and backward in NumPy at a chosen dtype, and its fault models -------------------------------------------------------------------------
def emulate(ref, theta, obs, acts, adv, ret, old_nlp, old_v, cr, mask, dtype, fault=None, padded=True, nudge=None):
    """ref.forward and ref.loss_grad's expressions at `dtype` (float64: must equal them; float32: what a correct kernel may compute), in their operand order.
    Returns dict(logits, v, nlp_all [n, A] (inf on forbidden ones), nlp, ent (rows), losses [5], grad [P]).
    fault: one of FAULTS --
      max_all        the row maximum runs over every category of the component, allowed or not
      pad0_in_max    a padding column (logit 0: zero weights, zero bias) takes part in the maximum (padded: the head has such a column)
      no_max_sub     exp(l) instead of exp(l - max)
      act_unchecked  the chosen action's probability is read by a one-hot product over exp(a0) of EVERY lane, forbidden ones included, without the allowed check
      ent_forbidden  the entropy term is evaluated on every column and multiplied by the 0 / 1 mask
    nudge: a RandomState; every row's neglogp is moved to the next float32 up or down at random -- another correct kernel, whose reduction rounds the other way"""
    F = dtype
    nvec = nvec_of(ref)
    off = offsets(nvec)
    n = len(obs)
    rows = np.arange(n)
    th = np.asarray(theta, F)
    T = lambda name: ref.t(name, th)
    L = len(ref.hidden)
    acts = np.asarray(acts).astype(np.int64).reshape(n, len(nvec))
    adv, ret, old_nlp, old_v = [np.asarray(x, F) for x in (adv, ret, old_nlp, old_v)]
    x = np.asarray(obs, F)
    hs = {"pi": [x], "vf": [x]}
    for tw in ("pi", "vf"):
        for l in range(L):
            hs[tw].append(np.tanh(hs[tw][-1] @ T("%s_fc%d/w" % (tw, l)) + T("%s_fc%d/b" % (tw, l))))
    logits = hs["pi"][-1] @ T("pi/w") + T("pi/b")
    v = (hs["vf"][-1] @ T("vf/w")).reshape(-1) + T("vf/b")[0]
    okall = np.ones(logits.shape, bool) if mask is None else (np.asarray(mask) != 0)
    comps = []
    nlp, ent = None, None
    nlp_all = np.full(logits.shape, np.inf, F)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        for k in range(len(nvec)):
            s = slice(int(off[k]), int(off[k + 1]))
            l, ok = logits[:, s], okall[:, s]
            m = (l if fault == "max_all" else np.where(ok, l, F(-np.inf))).max(1, keepdims=True)
            if fault == "pad0_in_max" and padded:
                m = np.maximum(m, F(0.0))
            if fault == "no_max_sub":
                m = np.zeros_like(m)
            a0 = l - m
            ex_raw = np.exp(a0)
            ex = np.where(ok, ex_raw, F(0.0))
            z = ex.sum(1, keepdims=True, dtype=F)
            lz = np.log(z)
            p = ex / z
            if fault == "ent_forbidden":
                terms = ok.astype(F) * ((ex_raw / z) * (lz - a0))
            else:
                terms = np.where(ok, p * (lz - a0), F(0.0))
            Hk = terms.sum(1, dtype=F)
            nk = lz[:, 0] - a0[rows, acts[:, k]]
            nlp_all[:, s] = np.where(ok, lz - a0, F(np.inf))
            nlp = nk if nlp is None else nlp + nk
            ent = Hk if ent is None else ent + Hk
            onehot = np.zeros(l.shape, F)
            onehot[rows, acts[:, k]] = 1
            comps.append((s, ok, a0, ex_raw, z, lz, p, Hk, onehot))
        if nudge is not None:
            nlp = np.nextafter(nlp, np.where(nudge.uniform(size=n) < 0.5, F(-np.inf), F(np.inf)).astype(F))
        crF = F(cr)
        lo, hi = F(1.0) - crF, F(1.0) + crF
        ratio = np.exp(old_nlp - nlp)
        rmin = np.minimum(ratio, hi)
        rclip = np.maximum(rmin, lo)
        m1, m2 = -adv * ratio, -adv * rclip
        sel = (m1 >= m2).astype(F)
        pas = (rmin >= lo).astype(F) * (ratio <= hi).astype(F)
        g = F(1.0) / F(n)
        d_ratio = (-adv) * g * sel + (-adv) * g * (F(1.0) - sel) * pas
        d_nlp = -(d_ratio * ratio)
        ec = F(ref.ent)
        dl = np.zeros(logits.shape, F)
        for s, ok, a0, ex_raw, z, lz, p, Hk, onehot in comps:
            if fault == "act_unchecked":
                p_act = (onehot * (ex_raw / z)).sum(1, keepdims=True, dtype=F)
                p = np.where(onehot != 0, p_act, p)
            # d (nlp) / d l = p - onehot; d (-H) / d l = p ((a0 - lz) + H)   [H = sum p (lz - a0)]
            dl[:, s] = np.where(ok, d_nlp[:, None] * (p - onehot) + ec * g * (p * ((a0 - lz) + Hk[:, None])), F(0.0))
        # value loss: 0.5 mean max((v - R)^2, (vclip - R)^2), vclip = vo + max(min(v - vo, cr), -cr); TF's tie rules as in the references
        dvo = v - old_v
        inner = np.where(dvo <= crF, dvo, crF)
        vclip = old_v + np.where(inner >= -crF, inner, -crF)
        pass_v = (dvo <= crF).astype(F) * (inner >= -crF).astype(F)
        s1, s2 = (v - ret) ** 2, (vclip - ret) ** 2
        selv = (s1 >= s2).astype(F)
        dv = F(ref.vfc) * F(0.5) * g * (selv * F(2.0) * (v - ret) + (F(1.0) - selv) * F(2.0) * (vclip - ret) * pass_v)
        losses = np.array([np.maximum(m1, m2).mean(dtype=F), F(0.5) * np.maximum(s1, s2).mean(dtype=F), ent.mean(dtype=F),
                           F(0.5) * ((nlp - old_nlp) ** 2).mean(dtype=F), (np.abs(ratio - F(1.0)) > crF).mean()], np.float64)
        grad = np.zeros(ref.P, F)

        def put(name, val):
            o, shape = ref.offs[name]
            grad[o:o + int(np.prod(shape))] = np.asarray(val, F).reshape(-1)

        for tw, head_w, d_out in (("pi", "pi/w", dl), ("vf", "vf/w", dv[:, None])):
            h = hs[tw]
            put(head_w, h[-1].T @ d_out)
            put(head_w[:-1] + "b", d_out.sum(0, dtype=F))
            dh = d_out @ T(head_w).T
            for l in range(L - 1, -1, -1):
                dz = dh * (F(1.0) - h[l + 1] * h[l + 1])
                put("%s_fc%d/w" % (tw, l), h[l].T @ dz)
                put("%s_fc%d/b" % (tw, l), dz.sum(0, dtype=F))
                dh = dz @ T("%s_fc%d/w" % (tw, l)).T
    return dict(logits=logits, v=v, nlp_all=nlp_all, nlp=nlp, ent=ent, losses=losses, grad=grad.astype(np.float64))


def emulate_batch(ref, b, dtype=np.float32, fault=None, acts=None, nudge=None):
    return emulate(ref, b.theta, b.obs, b.train_acts if acts is None else acts, b.adv, b.ret, b.old_nlp, b.old_v, CR, b.mask, dtype, fault, nudge=nudge)


def emulated_act(ref, b, fault=None):
    """what an fp32 kernel returns from an act call: (sampled actions, deterministic actions, values, neglogp of the sampled ones), Gumbel term in fp32"""
    nvec = nvec_of(ref)
    e = emulate_batch(ref, b, np.float32, fault, acts=b.acts)
    lg = e["logits"]
    with np.errstate(divide="ignore"):
        pert = (lg - np.log(-np.log(b.u.astype(np.float32)))).astype(np.float32)
    okall = np.ones(lg.shape, bool) if b.mask is None else b.mask != 0
    off = offsets(nvec)
    a = np.stack([np.argmax(np.where(okall, pert, -np.inf)[:, int(off[k]):int(off[k + 1])], 1) for k in range(len(nvec))], 1)
    det = np.stack([np.argmax(np.where(okall, lg, -np.inf)[:, int(off[k]):int(off[k + 1])], 1) for k in range(len(nvec))], 1)
    e2 = emulate_batch(ref, b, np.float32, fault, acts=a)
    return a.astype(np.float32), det.astype(np.float32), e["v"], e2["nlp"]


def emulated_train(ref, b, fault=None, dtype=np.float32, nudge=None):
    """what an fp32 kernel leaves after one train step: dict(losses, grad, norm, theta, m)"""
    e = emulate_batch(ref, b, dtype, fault, nudge=nudge)
    theta, m, norm = adam_after(ref, b.theta, e["grad"])
    return dict(losses=e["losses"], grad=e["grad"], theta=theta, m=m, norm=norm)


# ---- the assertions of part 1: the GPU tests and the CPU tests of their teeth call the same functions -----------------------------------------------------------
def close(a, b, rtol=1e-4, atol=1e-5, msg=""):
    np.testing.assert_allclose(a, b, rtol=rtol, atol=atol, err_msg=msg)


def single_rows(nvec, mask):
    """rows whose mask leaves one category in EVERY component"""
    if mask is None:
        return np.zeros(0, bool)
    off = offsets(nvec)
    return np.all([mask[:, int(off[k]):int(off[k + 1])].sum(1) == 1 for k in range(len(nvec))], axis=0)


def check_act(b, case, a, det, v, nlp, tag, nlp_extra=0.0, margin=TIE, exact_single=True):
    """sampled and deterministic actions, forbidden actions, ties, neglogp of the chosen action, value, single allowed category, finiteness.
    det None: the call has no deterministic form (the host-Env step).  margin: pairs whose two best entries are closer than this may go either way
    (part 1: TIE; part 2: 2 LOGIT_TOL, the clear-margin rule of tests/test_narrow_categorical.py).  nlp_extra: part 2's allowance beside the usual tolerance.
    exact_single=False: a row with one allowed category is held to |neglogp| <= 1e-6, the rule of tests/test_action_mask.py, instead of to exactly 0."""
    nvec, K, n = b.nvec, b.K, b.n
    off = offsets(nvec)[:-1]
    a = np.asarray(a).reshape(n, K)
    assert np.isfinite(a).all() and np.isfinite(v).all() and np.isfinite(nlp).all(), "%s: a non-finite act output" % tag
    ai = a.astype(np.int64)
    assert np.all(a == ai) and ai.min() >= 0 and np.all(ai < np.asarray(nvec)), "%s: not category indices" % tag
    if b.mask is not None:
        assert np.all(np.take_along_axis(b.mask, ai + off, 1) != 0), "%s: a forbidden category was sampled" % tag
    tie = top2_gap(nvec, b.pert) < margin
    bad = (ai != b.acts) & ~tie
    assert not bad.any(), "%s sampled actions: %d (row, component) pairs differ (first %s)" % (tag, bad.sum(), np.argwhere(bad)[:5].tolist())
    if det is not None:
        det = np.asarray(det).reshape(n, K)
        di = det.astype(np.int64)
        assert np.all(det == di) and di.min() >= 0 and np.all(di < np.asarray(nvec)), "%s: deterministic actions are not category indices" % tag
        x = b.logits if b.mask is None else np.where(b.mask != 0, b.logits, -np.inf)
        if b.mask is not None:
            assert np.all(np.take_along_axis(b.mask, di + off, 1) != 0), "%s: a forbidden category is the deterministic action" % tag
        gap = top2_gap(nvec, x)
        if case in ("ties", "two_ties"):
            np.testing.assert_array_equal(di, b.det, err_msg="%s: on a tie the deterministic action is the lowest allowed index" % tag)
        exact = gap == 0                                    # an exactly tied component in any case (fh_beside_ties' component 1): the same rule, no near-tie excuse
        np.testing.assert_array_equal(di[exact], b.det[exact], err_msg="%s: on an exact tie the deterministic action is the lowest allowed index" % tag)
        bad = (di != b.det) & ~(gap < margin)
        assert not bad.any(), "%s deterministic actions: %d pairs differ (first %s)" % (tag, bad.sum(), np.argwhere(bad)[:5].tolist())
    want = neglogp_of(nvec, b.logits, ai, b.mask)
    err = np.abs(nlp - want)
    assert np.all(err <= np.maximum(1e-5 * K + 1e-4 * np.abs(want), nlp_extra)), "%s neglogp: largest error %.3g at row %d (%.9g against %.12g)" % (
        tag, err.max(), err.argmax(), nlp[err.argmax()], want[err.argmax()])
    close(v, b.v, msg=tag + " value")
    one = single_rows(nvec, b.mask)
    if one.any() and exact_single:
        np.testing.assert_array_equal(nlp[one], 0.0, err_msg="%s: a row with one allowed category has neglogp exactly 0" % tag)
    elif one.any():
        assert np.all(np.abs(nlp[one]) <= 1e-6), (tag, nlp[one])


def check_train(ref, b, got, want, tag, ent_extra=0.0, grad_l2=None):
    """the five loss columns, gradient, global norm, theta and Adam m of tests/test_discrete_policy.test_three_train_steps_match_reference (entropy's absolute
    tolerance times K as in tests/test_multi_discrete.py), the exactly zero policy trunk and forbidden columns, finiteness, the single-category entropy.
    got / want: dict(losses, grad, norm, theta, m).  Part 2: ent_extra beside the entropy's usual tolerance; grad_l2: the gradient by its relative L2 error."""
    n, K = b.n, b.K
    for k in ("losses", "grad", "norm", "theta", "m"):
        assert np.isfinite(got[k]).all(), "%s: %s is not finite" % (tag, k)
    gl, wl = np.asarray(got["losses"], np.float64), want["losses"]
    close(gl[:2], wl[:2], rtol=1e-4, atol=1e-6, msg=tag + " pg / vf loss")
    assert abs(gl[2] - wl[2]) <= max(1e-6 * K + 1e-4 * abs(wl[2]), ent_extra), "%s entropy: %.9g against %.12g" % (tag, gl[2], wl[2])
    close(gl[3], wl[3], rtol=1e-4, atol=1e-6, msg=tag + " approxkl")
    assert abs(gl[4] - wl[4]) <= 1.0 / n + 1e-6, (tag, "clipfrac", gl[4], wl[4])
    grad, ref_grad = np.asarray(got["grad"], np.float64), want["grad"]
    gs = np.abs(ref_grad).max()
    if grad_l2 is None:
        close(grad, ref_grad, rtol=2e-4, atol=2e-6 * gs, msg=tag + " grad")
        close(got["theta"], want["theta"], rtol=1e-4, atol=2e-6, msg=tag + " theta")
        close(got["m"], want["m"], rtol=2e-4, atol=1e-7 * max(1.0, gs), msg=tag + " adam m")
    else:
        l2 = np.linalg.norm(grad - ref_grad) / np.linalg.norm(ref_grad)
        assert l2 <= grad_l2, "%s grad: relative L2 error %.3g (bound %.3g)" % (tag, l2, grad_l2)
    close(got["norm"], want["norm"], rtol=1e-4, msg=tag + " norm")
    if not np.any(ref.t("pi/w", b.theta)):
        for name, _ in ref.specs:
            if name.startswith("pi_fc"):
                x = ref.t(name, grad)
                np.testing.assert_array_equal(x, np.zeros(x.shape), err_msg="%s: pi/w = 0, so the gradient of %s is exactly zero" % (tag, name))
    if b.mask is not None:
        dead = np.all(b.mask == 0, axis=0)
        np.testing.assert_array_equal(ref.t("pi/b", grad)[dead], 0.0, err_msg=tag + ": pi/b gradient of a column every row forbids")
        np.testing.assert_array_equal(ref.t("pi/w", grad)[:, dead], 0.0, err_msg=tag + ": pi/w gradient of a column every row forbids")
    if single_rows(b.nvec, b.mask).all() and b.mask is not None:
        assert gl[2] == 0.0, "%s: rows with one allowed category contribute exactly 0 entropy (%.9g)" % (tag, gl[2])


def part2_bounds(ref, b):
    """(neglogp allowance, entropy allowance, gradient relative-L2 bound, the three measured emulation errors): PART2_FACTOR x what emulate(float32) shows against
    the float64 reference on the same rows; the gradient's bound is never tighter than the usual 2e-4, the other two are used beside the usual tolerances"""
    e32, e64 = emulate_batch(ref, b, np.float32), emulate_batch(ref, b, np.float64)
    ok = np.isfinite(e64["nlp_all"])
    e_nlp = float(np.abs(np.where(ok, e32["nlp_all"].astype(np.float64) - np.where(ok, e64["nlp_all"], 0.0), 0.0)).max())
    e_ent = float(abs(e32["losses"][2] - e64["losses"][2]))
    e_l2 = float(np.linalg.norm(e32["grad"] - e64["grad"]) / np.linalg.norm(e64["grad"]))
    return PART2_FACTOR * e_nlp, PART2_FACTOR * e_ent, max(PART2_FACTOR * e_l2, 2e-4), (e_nlp, e_ent, e_l2)
