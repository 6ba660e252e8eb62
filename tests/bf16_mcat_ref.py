"""float64 reference of the multi-categorical head of the bf16 path (bf16_sample_kernel / bf16_loss_kernel<mcat[,mask]>, ppo_cpp_amd/csrc/ppo_bf16.hpp) from the
head's own logits.  Plain NumPy, no GPU.  It does NOT restate the head: every formula and every bound is tests/bf16_cat_ref.py's (imported unchanged), applied to the
columns [o_k, o_k + n_k) of one component at a time, and the components' values are added in component order.  tests/test_bf16_multi_categorical.py cross-checks
the result against tests/multi_categorical_ref.MultiCatRef (float64 NumPy forward, torch float64 autograd of the stable-baselines expressions).

Actions are [n, K], column k the index WITHIN component k; masks and uniforms keep [n, A], A = sum(nvec).

HOW A ROW TOTAL GOES THROUGH THE ONE-COMPONENT FUNCTIONS.  bf16_cat_ref.loss and emu_loss_dlogits_f32 form the surrogate from THEIR neglogp and the old_neglogp they are
given.  For component k they are given  old_k = old_neglogp - sum_{i != k} neglogp_i  (float64), so that  neglogp_k - old_k = neglogp - old_neglogp: ratio, d_nlp, policy
loss, approxkl and clipfrac are the row's own, and d logits of the component's columns is d_nlp (p - 1_a) + ent_coef g p ((a0 - log z_k) + H_k) with the entropy H_k
of that component -- the kernel's expression (include/ppo_hip.h).

BOUNDS.  A per-element bound is bf16_cat_ref's; a row total's bound (neglogp, entropy) is the sum of its components' bounds.  ONE step is derived here, by hand, on
top of bf16_cat_ref: that module's loss() bounds the ratio with the E_nlp of the neglogp IT formed, which here is one component's, while the kernel's ratio carries the
error of the row total.  bf16_cat_ref.loss lets its E_nlp enter linearly -- the ratio's relative error r_r = E_nlp + U |dk| + 4 U, in E_dl through |T1| r_r, in the
policy-loss rows through |pg| r_r, in the approxkl rows through 2 |dk| E_nlp -- so loss() below ADDS the other components' E_nlp through the same three factors:
|T1| (E_nlp - E_nlp_k) to E_dl, mean |pg| (E_nlp - E_nlp_0) to the policy-loss term, mean |dk| (E_nlp - E_nlp_0) to approxkl.  That widens those bounds (never narrows
them) to what the row total's E_nlp gives.  T1 is read off a second bf16_cat_ref.loss call without the entropy term (that module does not return it), which doubles the
reference's cost per component; a one-component head adds nothing and skips the call.
"""
import numpy as np

from tests import bf16_cat_ref as C
from tests import bf16_ref as R

U = R.U


def offsets(nvec):
    return np.concatenate([[0], np.cumsum(nvec)]).astype(np.int64)


def comps(nvec):
    off = offsets(nvec)
    return [(int(off[k]), int(off[k + 1])) for k in range(len(nvec))]


def cut(x, o, e):
    return None if x is None else np.asarray(x)[:, o:e]


def acts_of(act, nvec):
    n = np.shape(act)[0]
    return np.asarray(act).reshape(n, len(nvec))


def head(logits, nvec, mask=None):
    """bf16_cat_ref.head of every component, in component order"""
    return [C.head(cut(logits, o, e), cut(mask, o, e)) for o, e in comps(nvec)]


def entropy(logits, nvec, mask=None):
    tot = None
    for hd in head(logits, nvec, mask):
        tot = hd["H"] if tot is None else tot + hd["H"]
    return tot


def sample(logits, u, nvec, mask=None):
    """[n, K]: bf16_cat_ref's Gumbel argmax per component, as indices within the component"""
    return np.stack([C.argmax_lowest(C.perturbed(cut(logits, o, e), cut(u, o, e), cut(mask, o, e))[0]) for o, e in comps(nvec)], axis=1)


def deterministic(logits, nvec, mask=None):
    return np.stack([C.argmax_lowest(np.where(C.allowed(cut(logits, o, e), cut(mask, o, e)), np.asarray(cut(logits, o, e), np.float64), -np.inf)) for o, e in comps(nvec)], axis=1)


def nlp_rows(logits, act, nvec, mask=None):
    """(row totals of neglogp, their bound, per component [K][n] values, per component bounds)"""
    a = acts_of(act, nvec).astype(np.int64)
    rows = np.arange(a.shape[0])
    vals, Es = [], []
    for k, hd in enumerate(head(logits, nvec, mask)):
        vals.append(hd["nlp_all"][rows, a[:, k]])
        Es.append(C.nlp_bound(hd, a[:, k])[0])
    tot, E = vals[0], Es[0]
    for k in range(1, len(vals)):
        tot = tot + vals[k]; E = E + Es[k]
    return tot, E, vals, Es


def smallest_gap(logits, u, nvec, mask=None):
    """the smallest distance of the two best perturbed allowed logits over every (row, component)"""
    best = np.inf
    for o, e in comps(nvec):
        pl, _ = C.perturbed(cut(logits, o, e), cut(u, o, e), cut(mask, o, e))
        s = np.sort(pl, axis=1)[:, -2:]
        with np.errstate(invalid="ignore"):
            gap = np.where(np.isfinite(s[:, 0]), s[:, 1] - s[:, 0], np.inf)
        best = min(best, float(gap.min()))
    return best


# ---- comparison rules (the GPU tests and the planted-fault test call the same functions) ----------------------------------------------------------
def check_sampled(name, act, logits, u, nvec, mask=None):
    """every component of every row by bf16_cat_ref.check_sampled's rules -- an integer in [0, n_k), never forbidden, the float64 Gumbel argmax of the device's own
    logits over the component's allowed set, lowest index on a tie -- with the (row, component) pairs inside the fp32 bound of the perturbed logits left out: at
    most (n K) // 256 of them per call.  Returns how many were left out."""
    n = np.shape(logits)[0]
    K = len(nvec)
    act = np.asarray(act)
    assert act.shape == (n, K), "%s: actions are [n, K] = %s, got %s" % (name, (n, K), act.shape)
    left = 0
    for k, (o, e) in enumerate(comps(nvec)):
        lk, uk, mk = cut(logits, o, e), cut(u, o, e), cut(mask, o, e)
        left += C.check_sampled("%s component %d" % (name, k), act[:, k], lk, uk, mk, max_skip=1.0)      # (the per-case allowance is applied to the total below)
    print("%s: (row, component) pairs left out as fp32 near-ties: %d of %d" % (name, left, n * K))
    assert left <= (n * K) // 256, "%s: %d of %d (row, component) pairs are near-ties" % (name, left, n * K)
    return left


def check_det(name, det, logits, nvec, mask=None):
    n = np.shape(logits)[0]
    det = np.asarray(det)
    assert det.shape == (n, len(nvec)), "%s: deterministic actions are [n, K]" % name
    for k, (o, e) in enumerate(comps(nvec)):
        got = det[:, k]
        assert np.all(got == np.floor(got)) and got.min() >= 0 and got.max() < e - o, "%s component %d: not category indices in [0, %d)" % (name, k, e - o)
        C.check_det("%s component %d" % (name, k), got, cut(logits, o, e), cut(mask, o, e))


def check_nlp(name, nlp, logits, act, nvec, mask=None, rec=None):
    want, E, _, _ = nlp_rows(logits, act, nvec, mask)
    R.check_f32(name, nlp, want, E, rec=rec)


# ---- loss -------------------------------------------------------------------------------------------------------------------------------------------
def loss(logits, v, act, adv, ret, old_v, old_nlp, cr, vcr, voff, ent_coef, vf_coef, nvec, mask=None, exact_consts=False):
    """bf16_loss_kernel<mcat[,mask]> in float64: bf16_cat_ref.loss per component (see the module text for old_k), the d logits side by side, the row totals in component
    order.  Same keys as bf16_cat_ref.loss; H / E_H are the row totals, "H_k" the per-component entropies."""
    n, A = np.shape(logits)
    a = acts_of(act, nvec).astype(np.int64)
    old_nlp = np.asarray(old_nlp, np.float64)
    adv64 = np.asarray(adv, np.float64)
    nlp, E_nlp, nlp_k, E_nlp_k = nlp_rows(logits, a, nvec, mask)
    parts = []
    for k, (o, e) in enumerate(comps(nvec)):
        others = nlp - nlp_k[k]
        parts.append(C.loss(cut(logits, o, e), v, a[:, k], adv, ret, old_v, old_nlp - others, cr, vcr, voff, ent_coef, vf_coef, cut(mask, o, e), exact_consts))
    first = parts[0]
    dk = nlp - old_nlp
    ratio = first["ratio"]
    dls, Es, Hs = [], [], []
    H, E_H = None, None
    for k, (o, e) in enumerate(comps(nvec)):
        p = parts[k]
        # T1 = d_nlp (p - 1_a), the term the ratio's error enters: the same call without the entropy term leaves exactly it
        extra = 0.0
        if len(nvec) > 1:
            T1 = C.loss(cut(logits, o, e), v, a[:, k], adv, ret, old_v, old_nlp - (nlp - nlp_k[k]), cr, vcr, voff, 0.0, vf_coef, cut(mask, o, e), exact_consts)["dl"]
            extra = np.where(p["ok"], np.abs(T1) * (E_nlp - E_nlp_k[k])[:, None], 0.0)
        dls.append(p["dl"]); Es.append(p["E_dl"] + extra); Hs.append(p["H"])
        H = p["H"] if H is None else H + p["H"]
        E_H = p["E_H"] if E_H is None else E_H + p["E_H"]
    dl, E_dl = np.concatenate(dls, axis=1), np.concatenate(Es, axis=1)
    ok = np.concatenate([p["ok"] for p in parts], axis=1)
    rest = E_nlp - E_nlp_k[0]
    # the policy-loss rows max(-adv ratio, -adv clip(ratio)) from the ratio bf16_cat_ref.loss formed: only to weigh the other components' E_nlp (the terms' values are that function's)
    pg = np.maximum(-adv64 * ratio, -adv64 * np.maximum(np.minimum(ratio, 1.0 + cr), 1.0 - cr))
    terms = list(first["terms"])
    terms[0] = (terms[0][0], terms[0][1] + float((np.abs(pg) * rest).sum() / n))
    terms[3] = (terms[3][0], terms[3][1] + float((2 * np.abs(dk) * rest).sum() / n * 0.5))
    ent_mean = sum(p["terms"][2][0] for p in parts[1:]) if len(parts) > 1 else 0.0
    terms[2] = (terms[2][0] + ent_mean, sum(p["terms"][2][1] for p in parts))
    db = R.column_sums(dl, E_dl, n)
    return dict(dl=dl, E_dl=E_dl, dv=first["dv"], E_dv=first["E_dv"], nlp=nlp, E_nlp=E_nlp, ratio=ratio, terms=terms, db=db, db_v=first["db_v"], H=H, E_H=E_H, ok=ok, H_k=Hs)


def emu_loss_dlogits_f32(logits, act, adv, old_nlp, cr, ent_coef, nvec, mask=None, drop_entropy_of=None):
    """bf16_cat_ref.emu_loss_dlogits_f32 per component, side by side (old_k rounded to fp32: the emulation measures a rounding share, in NumPy's own orders).
    drop_entropy_of: the planted fault of the CPU test (that component's second term left out)"""
    a = acts_of(act, nvec).astype(np.int64)
    old_nlp = np.asarray(old_nlp, np.float64)
    nlp, _, nlp_k, _ = nlp_rows(logits, a, nvec, mask)
    out = []
    for k, (o, e) in enumerate(comps(nvec)):
        old_k = (old_nlp - (nlp - nlp_k[k])).astype(np.float32)
        out.append(C.emu_loss_dlogits_f32(cut(logits, o, e), a[:, k], adv, old_k, cr, ent_coef, cut(mask, o, e), drop_entropy=(drop_entropy_of == k)))
    return np.concatenate(out, axis=1)


def check_dlogits(name, q, lo, share_ref, rec=None, floor=0.0, normal=0.0):
    """bf16_cat_ref.check_dlogits on the whole row: forbidden columns exactly 0, the allowed ones by rules (1) and (2) of tests/bf16_ref.py (floor, normal: see there)"""
    C.check_dlogits(name, q, lo, share_ref, rec, floor, normal)


def synth_batch_from(obs, act, v, nlp, seed, cr):
    return C.synth_batch_from(obs, act, v, nlp, seed, cr)
