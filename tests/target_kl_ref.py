"""Reference for target-KL early stopping (ppo_set_target_kl): ppo_update as a manual minibatch loop over the oracle's pieces -- loss_grad, clip, adam,
adv_normalize for the Gaussian head (oracle/oracle.py), loss_grad + clip_adam of tests/categorical_ref.py / tests/masked_categorical_ref.py for the categorical
one -- that stops BEFORE the Adam step of the first minibatch whose approxkl (losses[3] = 0.5 * sum of squared log-ratios / n) exceeds the limit.  The rows are
gathered as tests/test_oracle.py::test_update_loop_equals_manual_minibatching does: out.row(perm[i]) = in.row(i) over the env-major rows, contiguous slices."""
import numpy as np

from oracle import oracle as o

FIELDS = ("obs", "actions", "values", "neglogp", "returns")


def flat_rows(ro, fields):
    """env-major flatten of [T, E, ...] rollout fields (runner.hpp:136-152)"""
    T, E = np.asarray(ro["values"]).shape
    return {k: np.swapaxes(np.asarray(ro[k]), 0, 1).reshape((E * T,) + np.asarray(ro[k]).shape[2:]) for k in fields}


def minibatches(ro, perms, nmb, fields):
    """the update's minibatches in order: dicts of the fields' rows"""
    flat = flat_rows(ro, fields)
    B = flat["values"].shape[0]
    M = B // nmb
    for perm in perms:
        shuf = {k: np.empty_like(v) for k, v in flat.items()}
        for k in flat:
            shuf[k][np.asarray(perm)] = flat[k]
        for s in range(0, B, M):
            yield {k: v[s:s + M] for k, v in shuf.items()}


def exceeds(kl, limit):
    """the decision, in fp32 like the device's: approxkl > limit; no limit (None) never stops"""
    return limit is not None and bool(np.float32(kl) > np.float32(limit))


def gaussian_update(orc, ro, perms, nmb, lr, cr, limit=None):
    """orc: oracle.Oracle (advanced in place).  Returns (rows of the computed train steps -- the triggering one included --, Adam steps applied)."""
    rows, applied = [], 0
    for sl in minibatches(ro, perms, nmb, FIELDS):
        adv = o.adv_normalize(sl["returns"], sl["values"])
        losses, grad = orc.loss_grad(sl["obs"], sl["actions"], adv, sl["returns"], sl["neglogp"], sl["values"], cr)
        rows.append(losses.copy())
        if exceeds(losses[3], limit):
            break
        g, _ = orc.clip(grad)
        orc.adam(g, lr)
        applied += 1
    return np.stack(rows), applied


def categorical_update(ref, ro, perms, nmb, lr, cr, limit=None):
    """ref: CatRef / MaskedCatRef (advanced in place); ro["masks"] [T, E, A] travels with the rows when present.  Advantages as CatRef.update normalises them."""
    masked = "masks" in ro
    rows, applied = [], 0
    for sl in minibatches(ro, perms, nmb, FIELDS + (("masks",) if masked else ())):
        adv = sl["returns"].astype(np.float32) - sl["values"].astype(np.float32)
        adv = (adv - adv.mean(dtype=np.float64)) / (adv.std(dtype=np.float64) + 1e-8)
        args = (sl["obs"], sl["actions"], adv, sl["returns"], sl["neglogp"], sl["values"], cr)
        losses, grad = ref.loss_grad(*args, sl["masks"]) if masked else ref.loss_grad(*args)
        rows.append(np.asarray(losses, np.float64).copy())
        if exceeds(losses[3], limit):
            break
        ref.clip_adam(grad, lr)
        applied += 1
    return np.stack(rows), applied


def pick_limit(kl, nmb, min_s=2, allow_epoch_boundary=False):
    """(s, limit): limit = the midpoint between max(kl[:s]) and kl[s] for the first s >= min_s, not at an epoch boundary, where kl[s] > 1.05 * max(kl[:s]) and no
    kl lies within 5 % of the limit; None when the run has no such step"""
    kl = np.asarray(kl, np.float64)
    for s in range(min_s, len(kl)):
        if s % nmb == 0 and not allow_epoch_boundary:
            continue
        top = kl[:s].max()
        if not kl[s] > 1.05 * top:
            continue
        limit = 0.5 * (top + kl[s])
        if np.any(np.abs(kl - limit) <= 0.05 * limit):
            continue
        return s, float(np.float32(limit))
    return None


def clear_of(kl, limit):
    """no computed approxkl within 5 % of the limit: the device's fp32 sums take the same decision"""
    kl = np.asarray(kl, np.float64)
    return not np.any(np.abs(kl - limit) <= 0.05 * limit)
