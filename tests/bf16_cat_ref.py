"""float64 reference of the categorical head of the bf16 path (bf16_sample_kernel / bf16_loss_kernel<cat[,mask]>, ppo_cpp_amd/csrc/ppo_bf16.hpp) from the
head's own logits, the bounds on the kernels' fp32 arithmetic, and the rules its outputs are compared by.  Plain NumPy, no GPU.  It extends tests/bf16_ref.py
(imported unchanged: U, check_bf16, check_f32, vf_loss_rows, column_sums) in that file's manner: every stage is fed the DEVICE's own inputs to it -- here the logits,
i.e. the head GEMM's partial products added in range order in fp32 (bf16_ref.head_sum_f32, the device's own sum bit for bit).

A mask is [n, A], non-zero = allowed; None = every category allowed.  S = the allowed set of a row.
    m = max_S l,  a0 = l - m,  z = sum_S exp(a0),  p = exp(a0) / z on S (0 elsewhere)
    neglogp = log z - a0_a          H = sum_S p (log z - a0)
    sample  = argmax_S (l - log(-log u)), lowest index on a tie;  deterministic = argmax_S l, likewise
    d l_j   = d_nlp (p_j - [j == a]) + ent_coef g p_j ((a0_j - log z) + H) on S, exactly 0 elsewhere       (g = 1 / n)

DERIVED BOUNDS (U = 2^-24 = one fp32 rounding; expf / logf: 2 ulp = 4 U relative, the figure tests/bf16_ref.py uses for them)
    a0        one subtraction of exact fp32 logits (the maximum is exact): U |a0|
    exp(a0)   relative: 4 U (expf) + U |a0| (the argument's absolute error)
    z         positive terms, at most two per lane and a 6-level butterfly = 7 additions on any term's path, say 8 U relative:
              r_z = sum_S p (4 U + U |a0|) + 8 U
    log z     E_lz = r_z + 4 U |log z|
    neglogp   E_nlp = E_lz + U |a0_a| + U |neglogp|                                          (the subtraction)
    p         r_p = 4 U + U |a0| + r_z + U                                                   (the division)
    H         E_H = sum_S [ p r_p |t| + p (E_lz + U |a0| + U |t|) + U p |t| ] + 8 U H,  t = log z - a0 >= 0            (8 additions again)
    d l       first term   |d_nlp| (p r_p + U |p - 1_a|) + |T1| (r_r + 4 U) + U |T1|      (r_r: the ratio's relative error, as bf16_ref.loss derives it)
              second term  s = (a0 - log z) + H:  E_s = U |a0| + E_lz + U |a0 - log z| + E_H + U |s|;   c p s:  c (p E_s + p r_p |s| + U p |s|) + 2 U |T2|
              their sum    U |d l|
    perturbed logit  l - log(-log u) with u an exact fp32: logf(u) 4 U relative, the outer logf sees that as 4 U absolute and adds 4 U |log(-log u)|,
              the subtraction U |pl|:  E_pl = U (4 + 4 |log(-log u)| + |pl|).  A row whose best two perturbed ALLOWED values are closer than
              E_pl(best) + E_pl(second) may go either way in fp32: such rows are left out of the action comparison (tie_rows), at most 1 row in 256.
No bound is taken from the device's output.
"""
import numpy as np

from tests import bf16_ref as R

U = R.U


def allowed(logits, mask):
    return np.ones(np.shape(logits), bool) if mask is None else (np.asarray(mask) != 0)


def head(logits, mask=None):
    """float64 (a0, z, lz, p, nlp_all, H) of every row; p is 0 and nlp_all +inf on the forbidden categories"""
    l = np.asarray(logits, np.float64)
    ok = allowed(l, mask)
    m = np.where(ok, l, -np.inf).max(1, keepdims=True)
    a0 = l - m
    e = np.where(ok, np.exp(np.where(ok, a0, 0.0)), 0.0)
    z = e.sum(1, keepdims=True)
    lz = np.log(z)
    p = e / z
    nlp_all = np.where(ok, lz - a0, np.inf)
    Hrow = np.where(ok, p * (lz - a0), 0.0).sum(1)
    return dict(ok=ok, a0=a0, z=z[:, 0], lz=lz[:, 0], p=p, nlp_all=nlp_all, H=Hrow)


def perturbed(logits, u, mask=None):
    """(l - log(-log u) in float64 with -inf on the forbidden categories, E_pl)"""
    l = np.asarray(logits, np.float64); u = np.asarray(u, np.float64)
    with np.errstate(divide="ignore"):
        gum = np.log(-np.log(u))
    pl = l - gum
    E = U * (4 + 4 * np.abs(gum) + np.abs(pl))
    ok = allowed(l, mask)
    return np.where(ok, pl, -np.inf), np.where(ok, E, 0.0)


def argmax_lowest(x):
    """argmax with the lowest index on a tie (np.argmax's rule, stated)"""
    x = np.asarray(x)
    best = x.max(1, keepdims=True)
    return np.argmax(x == best, axis=1)


def tie_rows(pl, E):
    """rows whose best two perturbed allowed values are within the bound of their fp32 evaluation"""
    order = np.argsort(-pl, axis=1, kind="stable")
    rows = np.arange(pl.shape[0])
    b, s = order[:, 0], order[:, 1]
    with np.errstate(invalid="ignore"):
        gap = pl[rows, b] - pl[rows, s]
    return np.isfinite(pl[rows, s]) & (gap <= E[rows, b] + E[rows, s])


def nlp_bound(hd, act):
    """E_nlp of every row for the actions `act` (int)"""
    rows = np.arange(len(act))
    p, a0 = hd["p"], np.where(hd["ok"], hd["a0"], 0.0)
    rz = (p * (4 * U + U * np.abs(a0))).sum(1) + 8 * U
    Elz = rz + 4 * U * np.abs(hd["lz"])
    nlp = hd["nlp_all"][rows, act]
    return Elz + U * np.abs(a0[rows, act]) + U * np.abs(nlp), rz, Elz


# ---- comparison rules (the GPU tests and the planted-fault test call the same functions) ----------------------------------------------------------
def check_sampled(name, act, logits, u, mask=None, max_skip=1.0 / 256):
    """the sampled action is the float64 Gumbel argmax of the device's own logits over the allowed set, lowest index on a tie; rows inside the fp32 bound of
    l - log(-log u) are left out (printed; at most max_skip of the rows); never a forbidden category, always an integer in [0, A)"""
    act = np.asarray(act); n, A = np.shape(logits)
    ai = act.astype(np.int64)
    assert act.shape == (n,) and np.all(act == np.floor(act)) and ai.min() >= 0 and ai.max() < A, "%s: not category indices in [0, %d)" % (name, A)
    ok = allowed(logits, mask)
    assert np.all(ok[np.arange(n), ai]), "%s: a forbidden category was sampled on rows %s" % (name, np.nonzero(~ok[np.arange(n), ai])[0][:5])
    pl, E = perturbed(logits, u, mask)
    want = argmax_lowest(pl)
    tie = tie_rows(pl, E)
    exact_tie = np.sort(pl, axis=1)[:, -1] == np.sort(pl, axis=1)[:, -2] if A > 1 else np.zeros(n, bool)
    skip = tie & ~exact_tie                                   # an exact tie has a rule (the lowest index) and is checked
    bad = (ai != want) & ~skip
    print("%s: rows left out as fp32 near-ties: %d of %d" % (name, int(skip.sum()), n))
    assert not bad.any(), "%s: %d rows differ from the float64 Gumbel argmax (first %s: device %s, reference %s)" % (name, bad.sum(), np.nonzero(bad)[0][:5], ai[bad][:5], want[bad][:5])
    assert skip.sum() <= max(0, int(np.floor(max_skip * n))), "%s: %d of %d rows are near-ties" % (name, skip.sum(), n)
    return int(skip.sum())


def check_det(name, det, logits, mask=None):
    """the deterministic action is the argmax of the (exact fp32) logits over the allowed set, lowest index on a tie: no tolerance"""
    l = np.where(allowed(logits, mask), np.asarray(logits, np.float64), -np.inf)
    want = argmax_lowest(l)
    got = np.asarray(det).astype(np.int64)
    assert np.all(np.asarray(det) == got), name
    bad = got != want
    assert not bad.any(), "%s: %d rows are not the lowest-index argmax of the logits (first %s: device %s, reference %s)" % (name, bad.sum(), np.nonzero(bad)[0][:5], got[bad][:5], want[bad][:5])


def check_nlp(name, nlp, logits, act, mask=None, rec=None):
    hd = head(logits, mask)
    ai = np.asarray(act).astype(np.int64)
    E, _, _ = nlp_bound(hd, ai)
    R.check_f32(name, nlp, hd["nlp_all"][np.arange(len(ai)), ai], E, rec=rec)


# ---- loss -------------------------------------------------------------------------------------------------------------------------------------------
def loss(logits, v, act, adv, ret, old_v, old_nlp, cr, vcr, voff, ent_coef, vf_coef, mask=None, exact_consts=False):
    """bf16_loss_kernel<cat[,mask]> in float64 from the kernel's own head sums (logits [n][A], v [n]): per-row d logits / d v with bounds, the five loss terms
    {pg, vf, entropy, approxkl, clipfrac} with bounds, the pi/b and vf/b gradients (sums of the UNROUNDED values) with bounds.
    exact_consts: 1 / n, ent_coef and vf_coef / 2 n as real numbers instead of the kernel's fp32 constants (the comparison with the float64 references)"""
    n, A = logits.shape
    adv, ret, old_v, old_nlp, v = [np.asarray(x, np.float64) for x in (adv, ret, old_v, old_nlp, v)]
    ai = np.asarray(act).astype(np.int64)
    rows = np.arange(n)
    g = 1.0 / n if exact_consts else float(np.float32(1.0) / np.float32(n))
    hd = head(logits, mask)
    ok, p, lz, Hrow = hd["ok"], hd["p"], hd["lz"], hd["H"]
    a0 = np.where(ok, hd["a0"], 0.0)
    Enlp, rz, Elz = nlp_bound(hd, ai)
    nlp = hd["nlp_all"][rows, ai]
    dk = nlp - old_nlp
    ratio = np.exp(-dk)
    lo, hi = 1.0 - cr, 1.0 + cr
    rmin = np.minimum(ratio, hi); rclip = np.maximum(rmin, lo)
    m1, m2 = -adv * ratio, -adv * rclip
    sel = (m1 >= m2) * 1.0
    pas = (rmin >= lo) * (ratio <= hi) * 1.0
    d_ratio = -adv * g * sel + -adv * g * (1 - sel) * pas
    d_nlp = -(d_ratio * ratio)
    rr = Enlp + U * np.abs(dk) + 4 * U
    onehot = np.zeros((n, A)); onehot[rows, ai] = 1.0
    c = (ent_coef if exact_consts else float(np.float32(ent_coef))) * g
    t = np.where(ok, lz[:, None] - a0, 0.0)
    rp = 5 * U + U * np.abs(a0) + rz[:, None]
    E_H = (p * rp * t + p * (Elz[:, None] + U * np.abs(a0) + U * t) + U * p * t).sum(1) + 8 * U * Hrow
    T1 = d_nlp[:, None] * (p - onehot)
    s = (a0 - lz[:, None]) + Hrow[:, None]
    T2 = c * p * s
    dl = np.where(ok, T1 + T2, 0.0)
    E_T1 = np.abs(d_nlp)[:, None] * (p * rp + U * np.abs(p - onehot)) + np.abs(T1) * (rr[:, None] + 4 * U) + U * np.abs(T1)
    E_s = U * np.abs(a0) + Elz[:, None] + U * np.abs(a0 - lz[:, None]) + E_H[:, None] + U * np.abs(s)
    E_T2 = c * (p * E_s + p * rp * np.abs(s) + U * p * np.abs(s)) + 2 * U * np.abs(T2)
    E_dl = np.where(ok, E_T1 + E_T2 + U * np.abs(dl), 0.0)
    gv = vf_coef * 0.5 * g if exact_consts else float(np.float32(np.float32(vf_coef) * np.float32(0.5)) * np.float32(g))
    lossv, dv, esum = R.vf_loss_rows(v, ret, old_v, vcr, voff, gv)
    mag = np.abs(v) + np.abs(old_v) + np.abs(ret) + vcr
    E_dv = 6 * U * gv * mag + 8 * U * np.abs(dv)
    E_lossv = 2 * esum * 3 * U * mag + 2 * U * lossv
    pg = np.maximum(m1, m2)
    cf = (np.abs(ratio - 1.0) > cr) * 1.0

    def mean_term(r_, E_rows, half=False):
        sm = r_.sum() / n * (0.5 if half else 1.0)
        E = (E_rows.sum() + 2 * n * U * np.abs(r_).sum()) / n * (0.5 if half else 1.0)
        return sm, E + 4 * U * abs(sm)
    terms = [mean_term(pg, np.abs(pg) * (rr + 2 * U)), mean_term(lossv, E_lossv, True), mean_term(Hrow, E_H),
             mean_term(dk * dk, 2 * np.abs(dk) * (Enlp + U * np.abs(dk)) + U * dk * dk, True), mean_term(cf, np.zeros(n))]
    db = R.column_sums(dl, E_dl, n)
    db_v = (dv.sum(), E_dv.sum() + 2 * n * U * np.abs(dv).sum())
    return dict(dl=dl, E_dl=E_dl, dv=dv, E_dv=E_dv, nlp=nlp, E_nlp=Enlp, ratio=ratio, terms=terms, db=db, db_v=db_v, H=Hrow, E_H=E_H, ok=ok)


def emu_loss_dlogits_f32(logits, act, adv, old_nlp, cr, ent_coef, mask=None, drop_entropy=False):
    """bf16_loss_kernel<cat[,mask]>'s d logits in NumPy fp32 arithmetic (every operation of the kernel's expression in fp32, NumPy's own summation order).
    drop_entropy: the planted fault of the CPU test (the second term left out)"""
    F = np.float32
    l = R.f32(logits); adv = R.f32(adv); old_nlp = R.f32(old_nlp)
    n, A = l.shape
    ok = allowed(l, mask)
    ai = np.asarray(act).astype(np.int64)
    rows = np.arange(n)
    m = np.where(ok, l, F(-np.inf)).max(1, keepdims=True)
    a0 = np.where(ok, l - m, F(0.0)).astype(F)
    ex = np.where(ok, np.exp(a0), F(0.0)).astype(F)
    z = ex.sum(1, dtype=F)
    lz = np.log(z)
    nlp = (lz - a0[rows, ai]).astype(F)
    p = (ex / z[:, None]).astype(F)
    Hrow = (p * (lz[:, None] - a0)).astype(F).sum(1, dtype=F)
    ratio = np.exp(old_nlp - nlp)
    lo, hi = F(1.0) - F(cr), F(1.0) + F(cr)
    rmin = np.minimum(ratio, hi); rclip = np.maximum(rmin, lo)
    g = F(1.0) / F(n)
    sel = ((-adv * ratio) >= (-adv * rclip)).astype(F)
    pas = (rmin >= lo).astype(F) * (ratio <= hi).astype(F)
    d_ratio = (-adv) * g * sel + (-adv) * g * (F(1.0) - sel) * pas
    d_nlp = -(d_ratio * ratio)
    onehot = np.zeros((n, A), F); onehot[rows, ai] = F(1.0)
    T1 = d_nlp[:, None] * (p - onehot)
    T2 = (F(ent_coef) * g) * (p * ((a0 - lz[:, None]) + Hrow[:, None]))
    dl = T1 if drop_entropy else T1 + T2
    return np.where(ok, dl, F(0.0)).astype(F)


def normal_size(lo, normal=0.0):
    """the allowed d logits of at least `normal` in size (0: every allowed one): the elements rule (2) counts"""
    return lo["ok"] & (np.abs(lo["dl"]) >= normal)


def check_dlogits(name, q, lo, share_ref, rec=None, floor=0.0, normal=0.0):
    """q [n][A]: the device's bf16 d logits as fp32.  Forbidden categories exactly 0; the allowed ones by rules (1) and (2) of tests/bf16_ref.py.
    floor, normal (tests/test_head_edges.py: logits spread by hundreds, where exp(a0) underflows): every bound gets `floor` (below the smallest normal float32 a
    term may be flushed to zero or keep only some of its bits), every allowed element must be inside its bracket, and rule (2) counts the elements of
    normal_size(lo, normal) only -- share_ref is then the emulation's share on those"""
    q = np.asarray(q, np.float64)
    ok = lo["ok"]
    assert not q[~ok].any(), "%s: %d non-zero d logits on forbidden categories" % (name, int(np.count_nonzero(q[~ok])))
    if not floor and not normal:
        R.check_bf16(name, q[ok], lo["dl"][ok], lo["E_dl"][ok], share_ref, rec)
        return
    outside = R.bf16_findings(q[ok], lo["dl"][ok], lo["E_dl"][ok] + floor, 0.0)[0]
    assert not outside.any(), "%s: %d of %d elements leave the bracket (first: device %.9g, float64 %.12g)" % (
        name, outside.sum(), outside.size, q[ok][outside][0], lo["dl"][ok][outside][0])
    sel = normal_size(lo, normal)
    if sel.any():
        R.check_bf16(name, q[sel], lo["dl"][sel], lo["E_dl"][sel] + floor, share_ref, rec)


def synth_batch_from(obs, act, v, nlp, seed, cr):
    """helpers.synth_minibatch_from's perturbations around given categorical outputs (actions are category indices), advantages normalised in NumPy"""
    from tests import helpers as H
    mb = H.synth_minibatch_from(obs, np.asarray(act, np.float32), np.asarray(v, np.float32), np.asarray(nlp, np.float32), seed, adv_normalized=False, cr=cr)
    adv = mb["advs"].astype(np.float64)
    mb["advs"] = ((adv - adv.mean()) / (adv.std() + 1e-8)).astype(np.float32)
    return mb
