"""Bounds of the wide categorical head of the bf16 path (bf16_{sample,loss,eval}_wide_kernel<EPT, MASK>), restated from tests/bf16_cat_ref.py (imported unchanged).

The arithmetic per element is that file's; only the SUMMATION PATH of a row sum differs: a lane adds its EPT elements in order (EPT - 1 additions on the longest
path, one more from the zero the sum starts at) and a 6-level butterfly follows: EPT + 6 additions where the 128-wide kernels have 7.  bf16_cat_ref charges 8 U for
its 7; here every row sum is charged d = (EPT - 1) U MORE, and d is carried through that file's derivation term by term (U = 2^-24):
    r_z, E_lz, E_nlp, r_p, r_r     + d each (z enters each once)
    E_H        + sum_S [p d t + p d] + d H = d (2 H + 1)                 (r_p and E_lz inside the sum, then the sum's own path; sum_S p t = H, sum_S p = 1)
    E_T1       + |d_nlp| p d + |T1| d  <=  2 d |adv| g ratio             (|d_nlp| <= |adv| g ratio, p <= 1, |p - 1_a| <= 1)
    E_s        + d + d (2 H + 1);    E_T2  + c p d (2 H + 2 + |s|)
    loss terms: pg |pg| d, entropy d (2 H + 1), approxkl 2 |dk| d  per row, averaged as mean_term does
At A = 1024 (EPT 16) with a logit spread within 20 this gives E_nlp < 2e-5 and E_H < 1e-4: |log z| <= log 1024 + 20 < 27 and |a0| <= 20, so
E_nlp <= (4 + 20 + 8 + 15) U + 4 U 27 + 20 U + 47 U < 225 U = 1.4e-5, and E_H <= (2 H + 1) (r_p + E_lz + ..) with H <= log 1024 stays under 1600 U = 9.6e-5.
No bound is taken from the device's output."""
import numpy as np

from tests import bf16_cat_ref as C

U = C.U


def ept_of(A):
    return 4 if A <= 256 else 8 if A <= 512 else 16


def nlp_bound(logits, act, mask=None):
    """(float64 neglogp of `act`, E_nlp) of every row"""
    hd = C.head(logits, mask)
    ai = np.asarray(act).astype(np.int64)
    return hd["nlp_all"][np.arange(len(ai)), ai], C.nlp_bound(hd, ai)[0] + (ept_of(np.shape(logits)[1]) - 1) * U


def loss(logits, v, act, adv, ret, old_v, old_nlp, cr, ent_coef, vf_coef, mask=None):
    """bf16_cat_ref.loss with every bound that a row sum enters widened as derived above"""
    n, A = logits.shape
    lo = C.loss(logits, v, act, adv, ret, old_v, old_nlp, cr, cr, 0.0, ent_coef, vf_coef, mask)
    d = (ept_of(A) - 1) * U
    g = float(np.float32(1.0) / np.float32(n))
    hd = C.head(logits, mask)
    p, H = hd["p"], hd["H"][:, None]
    s = np.where(lo["ok"], (hd["a0"] - hd["lz"][:, None]) + H, 0.0)
    c = float(np.float32(ent_coef)) * g
    extra = 2 * d * (np.abs(np.asarray(adv, np.float64)) * g * lo["ratio"])[:, None] + c * p * d * (2 * H + 2 + np.abs(s))
    lo["E_dl"] = lo["E_dl"] + np.where(lo["ok"], extra, 0.0)
    lo["E_nlp"] = lo["E_nlp"] + d
    lo["E_H"] = lo["E_H"] + d * (2 * lo["H"] + 1)
    lo["db"] = (lo["db"][0], lo["db"][1] + np.where(lo["ok"], extra, 0.0).sum(0))
    dk = lo["nlp"] - np.asarray(old_nlp, np.float64)
    t = lo["terms"]
    pg = np.maximum(-np.asarray(adv, np.float64) * lo["ratio"], -np.asarray(adv, np.float64) * np.clip(lo["ratio"], 1 - cr, 1 + cr))
    more = [np.abs(pg).mean() * d, 0.0, (d * (2 * lo["H"] + 1)).mean(), np.abs(dk).mean() * d, 0.0]
    lo["terms"] = [(t[k][0], t[k][1] + more[k]) for k in range(5)]
    return lo
