"""float64 reference of every stage of the bf16 matrix-core path (ppo_cpp_amd/csrc/ppo_bf16.hpp), and the rules its outputs are compared by.
Plain NumPy, no GPU.  tests/test_bf16_stages.py feeds every stage the DEVICE's own inputs to that stage ("teacher forcing"): given its bf16
operands a stage's output is determined up to fp32 accumulation error, so errors neither cascade nor hide behind bf16's operand error.

Rounding points of the path (each verified against the code; `rnd` below is rne_bf16 on the device's arithmetic, `identity` for the fp32 oracle's):
    x0       = rnd(obs)                                  bf16_stage_kernel / bf16_stage4_kernel (act path: rnd(normalised fp32 obs))
    theta_bf = rnd(theta)                                bf16_cast_kernel after an upload, bf16_reduce_adam_kernel / adam_kernel after a step
    h_l      = rnd(tanh(h_{l-1} W_bf + b_fp32))          gb_epilogue_bf16<GEPI_TANH>
    heads    = h_L W_bf + b  (fp32, GB_HEAD_SPLIT ranges) bf16_heads_kernel; consumers add the ranges in range order in fp32 (head_sum)
    dhead    = rnd(d loss / d head)                      bf16_loss_kernel; its bias / logstd sums are taken from the UNROUNDED fp32 values
    dy_{l-1} = rnd((dy_l W_bf^T) .* (1 - h_{l-1}^2))      gb_epilogue_bf16<GEPI_TANHGRAD>; bias sums (csum) from the unrounded fp32 products
    dW_l     = h_{l-1}^T dy_l  (fp32)                    gemm_dw_bf16_kernel slabs + bf16_grad_reduce_kernel / bf16_reduce_adam_kernel
    clip + Adam in fp32                                  bf16_reduce_adam_kernel / adam_kernel (adam_element)

HOW OUTPUTS ARE COMPARED (stated once, used everywhere)

U = 2^-24 is one fp32 rounding (half an ulp, relative).

(1) bf16 outputs, rigorous bracket (check_bf16).  y = the float64 value before rounding, E = a bound on the kernel's fp32 error of that element.
    Round-to-nearest-even is monotone, so  rne(y - E) <= q <= rne(y + E).  E for a reduction of padded length K: bf16 x bf16 products are exact
    in fp32, only the K additions round; the matrix unit's internal rounding is not documented, so 2 units per addition:
        E_sum = 2 K U (sum|a||b| + |bias|)            (sum|a||b| from a second float64 matmul)
    propagated through the epilogue with its derivative -- (1 - h^2) for tanh (plus the second-order term 0.77 E^2, max|tanh''| = 0.77),
    |1 - h^2| for TanhGrad -- plus the epilogue's own roundings:
      tanh = 1 - 2 rcp(exp2(x 2log2e) + 1), TANH_ALLOW = 10 U absolute: argument (constant, bias product, fma: 3 U |x|, times the slope:
      |x| (1 - h^2) <= 0.45 -> 1.4 U), exp2 1 ulp (= 2 U relative on e; dh/de e = 2 e / (e + 1)^2 <= 1/2 -> 1 U), e + 1 (2 r U <= 2 U),
      rcp 1 ulp (2 r 2 U <= 4 U), final fma (|h| U <= 1 U): 9.4 U.
      TanhGrad = acc * (1 - h * h): three roundings, 4 U |y|.
(2) bf16 outputs, exact-rounding rate (also check_bf16).  The bracket is about +-1 bf16 ulp wide at K = 1024, so alone it would accept truncation
    or a rounding taken at the wrong point: the share of elements with q != rne(y) is capped as well.  The cap is a condition set from the reference
    alone: the same stage is emulated on the CPU in NumPy fp32 arithmetic on the same bf16 operands (emu_* below) and its own mismatch share s against
    rne(y) is measured; the cap is 10 s (the factor: another summation order, the hardware tanh), with s never taken below 1 / N (N elements cannot
    resolve a smaller share: "none of N" means "< 1 / N").  A systematic fault (truncation, a double rounding) gives tens of percent.
(3) fp32 outputs (check_f32): per element |out - ref| <= E with the same derived bound (M rows in the place of K for dW and the bias sums, plus the
    assembly's additions); per tensor the relative L2 error against the float64 value is at most 10 x what the CPU fp32 emulation shows on the same
    inputs (never below L2_FLOOR = 2 U: one rounding of the output itself).
No bound is taken from the device's output.

CPU emulation on the reference's own chain (cpu_chain_shares; the six shapes of tests/test_bf16_stages.py::CASES), measured with NumPy's fp32 matmul:
                                         mismatch share of rne(fp32 emulation) vs rne(float64)        relative L2 error of the fp32 emulation
    case (hidden, O, A, n)               hidden fwd   backward dy   dhead (loss)                      head sums   bias sums   dW
    (256, 128), 18, 18, 130              4.2e-4       6.0e-5        4.3e-4                            6.4e-8      4.2e-7      8.9e-8
    (384,), 40, 7, 640                   3.1e-4       0 of 2.5e5    0 of 4480                         1.3e-7      3.6e-7      1.4e-7
    (128, 2048), 18, 18, 256             6.9e-4       1.2e-4        2.2e-4                            1.8e-7      4.6e-7      1.1e-7
    (1280,), 18, 70, 128                 7.4e-4       6.1e-6        5.6e-4                            1.5e-7      2.4e-7      8.9e-8
    (1024, 512), 300, 100, 1000          2.3e-4       8.2e-5        9.3e-4                            1.1e-7      1.1e-6      1.6e-7
    (512, 512), 64, 18, 2048             2.9e-4       8.9e-5        1.6e-4                            1.1e-7      7.5e-7      1.7e-7
i.e. order 1e-4 to 1e-3 where a systematic fault gives tens of percent.  (The hidden layers' share is that of the epilogue's tanh FORM, emu_tanh_f32: with a
correctly rounded tanh in its place the same emulation shows 2e-5 to 1.5e-4.)  CPU_SHARES / CPU_L2 below record twice the largest figure of each column (the factor two: another
BLAS blocking sums in another order), and tests/test_bf16_stages.py::test_cpu_emulation_shares_stay_under_the_recorded_figures holds the emulation to them, so the
caps cannot rot.  CHOSEN CAPS against the device: share <= 10 x max(s, 1 / N) and relative L2 <= 10 x max(e, 2 U), with s / e the emulation's own figure on the
device's inputs to that stage -- at most 10 x the recorded figures' scale, i.e. shares of a few 1e-3 and relative L2 errors of a few 1e-6.
OBSERVED on an MI355X (largest over every GPU test of tests/test_bf16_stages.py, where the table per stage is): mismatch shares hidden forward 2.1e-3 (cap 2.1e-2),
dhead 8.7e-4, backward 9.7e-5 (cap 1.2e-3); relative L2 head sums 1.5e-7, bias sums 5.7e-7, dW 1.4e-7 (caps 1.7e-6 .. 1.7e-5); no element needed more than 0.13 E.
"""
import numpy as np

U = 2.0 ** -24
TANH_ALLOW = 10 * U
L2_FLOOR = 2 * U
HALF_LOG_2PI = float(np.float32(0.9189385175704956))
HALF_LOG_2PIE = float(np.float32(1.4189385175704956))
RATE_FACTOR = 10.0
L2_FACTOR = 10.0

# twice the largest mismatch share / relative L2 error the CPU fp32 emulation showed per stage over the six CASES (the table above)
CPU_SHARES = {"hidden": 1.5e-3, "dy": 2.5e-4, "dhead": 2e-3}
CPU_L2 = {"heads": 4e-7, "dbias": 2.2e-6, "dw": 3.4e-7}


def ru(x, m):
    return (x + m - 1) // m * m


# ---- bf16 ------------------------------------------------------------------------------------------------------------------------------------
def rne_bf16(x):
    """fp32 -> bf16 round-to-nearest-even, returned as fp32 (NaN stays NaN: the carry cannot leave the mantissa of a quiet NaN's payload here)"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    r = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16) & 0xFFFFFFFF
    out = r.astype(np.uint32).view(np.float32).reshape(x.shape)
    return np.where(np.isnan(x), x, out)


def trunc_bf16(x):
    """the FAULT the rate check exists for: the low 16 bits dropped"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    return (x.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32).reshape(x.shape)


def identity(x):
    return x


def bf16_bits(x):
    """uint16 bit patterns of fp32 values that ARE bf16 values"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    u = x.view(np.uint32)
    assert not np.any(u & np.uint32(0xFFFF)), "not a bf16 value"
    return (u >> np.uint32(16)).astype(np.uint16).reshape(x.shape)


def from_bits(u16):
    """bf16 bit patterns -> fp32"""
    return (np.ascontiguousarray(u16, dtype=np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32)


def r64(rnd, y):
    """a rounding applied to float64 values (through fp32, as the kernels' fp32 registers are), back in float64"""
    return np.asarray(rnd(np.asarray(y, np.float64).astype(np.float32)), np.float64)


# ---- comparison rules ---------------------------------------------------------------------------------------------------------------------------
class Record(dict):
    """observed figures per stage: the largest |q - y| in bracket units, mismatch shares, relative L2 errors (printed by the GPU tests)"""

    def note(self, name, **kw):
        cur = self.setdefault(name, {})
        for k, v in kw.items():
            cur[k] = max(cur.get(k, 0.0), float(v))


def bracket(y, E):
    y = np.asarray(y, np.float64); E = np.asarray(E, np.float64)
    return rne_bf16((y - E).astype(np.float32)).astype(np.float64), rne_bf16((y + E).astype(np.float32)).astype(np.float64)


def mismatch_share(q, y):
    return float(np.mean(np.asarray(q, np.float64) != rne_bf16(np.asarray(y, np.float64).astype(np.float32)).astype(np.float64)))


def bf16_findings(q, y, E, share_ref):
    """(elements outside the bracket, mismatch share, its cap, bracket units).  Bracket units: the largest share of E an element NEEDED -- where q != rne(y),
    the distance from y to the rounding boundary between rne(y) and q (their midpoint), over E; 0 where q == rne(y); beyond 1 the element leaves the bracket"""
    q = np.asarray(q, np.float64); y = np.asarray(y, np.float64)
    # (E is applied in float64 and the ends are rounded from fp32: add one fp32 rounding of y so that the conversion cannot cut the bracket short)
    E = np.asarray(E, np.float64) + U * np.abs(y)
    lo, hi = bracket(y, E)
    outside = ~((q >= lo) & (q <= hi))
    r = rne_bf16(y.astype(np.float32)).astype(np.float64)
    with np.errstate(invalid="ignore"):
        need = np.where(q != r, np.abs((q + r) / 2 - y), 0.0) / np.maximum(E, 1e-300)
    share = float(np.mean(q != r))
    cap = RATE_FACTOR * max(share_ref, 1.0 / q.size)
    return outside, share, cap, float(np.max(need)) if q.size else 0.0


def check_bf16(name, q, y, E, share_ref, rec=None):
    """rules (1) and (2): q = the device's bf16 output as fp32, y = the float64 value before rounding, E its derived error bound, share_ref = the CPU
    fp32 emulation's own mismatch share on the same inputs"""
    outside, share, cap, units = bf16_findings(q, y, E, share_ref)
    if rec is not None:
        rec.note(name, bracket_units=units, share=share, share_cap=cap)
    if outside.any():
        idx = np.argwhere(outside)
        i = tuple(idx[0])
        lo, hi = [float(np.ravel(b)[0]) for b in bracket(np.asarray(y, np.float64)[i], np.asarray(E, np.float64)[i] if np.ndim(E) else E)]
        raise AssertionError("%s: %d of %d elements leave the bracket; first at %s: device %.9g, float64 %.12g, bracket [%.9g, %.9g]"
                             % (name, idx.shape[0], outside.size, i, np.asarray(q)[i], np.asarray(y)[i], lo, hi))
    assert share <= cap, "%s: %.4g of the elements are not rne(y) (cap %.4g = %g x max(CPU fp32 emulation %.4g, 1 / %d))" % (name, share, cap, RATE_FACTOR, share_ref, np.asarray(q).size)


def rel_l2(out, ref):
    out = np.asarray(out, np.float64); ref = np.asarray(ref, np.float64)
    return float(np.linalg.norm(out - ref) / max(np.linalg.norm(ref), 1e-300))


def f32_findings(out, ref, E, l2_ref):
    out = np.asarray(out, np.float64); ref = np.asarray(ref, np.float64)
    E = np.broadcast_to(np.asarray(E, np.float64), ref.shape)
    bad = ~(np.abs(out - ref) <= E)
    units = float(np.max(np.abs(out - ref) / np.maximum(E, 1e-300))) if ref.size else 0.0
    return bad, rel_l2(out, ref), L2_FACTOR * max(l2_ref, L2_FLOOR), units


def check_f32(name, out, ref, E, l2_ref=None, rec=None):
    """rule (3).  l2_ref = the CPU fp32 emulation's relative L2 error on the same inputs (None: the per-element bound only -- scalars and short vectors)"""
    bad, l2, cap, units = f32_findings(out, ref, E, l2_ref or 0.0)
    if rec is not None:
        rec.note(name, bound_units=units, **({"rel_l2": l2, "rel_l2_cap": cap} if l2_ref is not None else {}))
    if bad.any():
        idx = np.argwhere(bad)
        i = tuple(idx[0])
        raise AssertionError("%s: %d of %d elements are further from the float64 value than the derived bound; first at %s: device %.9g, float64 %.12g, bound %.3g"
                             % (name, idx.shape[0], bad.size, i, np.asarray(out, np.float64)[i], np.asarray(ref, np.float64)[i],
                                np.broadcast_to(np.asarray(E, np.float64), np.shape(ref))[i]))
    if l2_ref is not None:
        assert l2 <= cap, "%s: relative L2 error %.4g (cap %.4g = %g x max(CPU fp32 emulation %.4g, 2 U))" % (name, l2, cap, L2_FACTOR, l2_ref)


# ---- stages: float64 value, derived bound ----------------------------------------------------------------------------------------------------------
def affine(a, w, bias=None):
    """(a w + bias, sum|a||w| + |bias|) in float64"""
    a = np.asarray(a, np.float64); w = np.asarray(w, np.float64)
    z = a @ w; s = np.abs(a) @ np.abs(w)
    if bias is not None:
        z = z + np.asarray(bias, np.float64); s = s + np.abs(np.asarray(bias, np.float64))
    return z, s


def stage_obs(obs, rows_pad, Kp0, rnd=rne_bf16):
    """bf16_stage_kernel / bf16_stage4_kernel: [rows_pad][Kp0], zero outside the n x O observations"""
    obs = np.asarray(obs, np.float32)
    x = np.zeros((rows_pad, Kp0), np.float32)
    x[:obs.shape[0], :obs.shape[1]] = rnd(obs)
    return x


def normalise_f32(raw, mean, var, eps, clip):
    """the act path's normalisation in the kernels' fp32 arithmetic: (x - mean) * (1 / sqrt(var + eps)), clipped (every operation correctly rounded)"""
    raw = np.asarray(raw, np.float32); mean = np.asarray(mean, np.float32); var = np.asarray(var, np.float32)
    sc = np.float32(1.0) / np.sqrt(var + np.float32(eps), dtype=np.float32)
    x = (raw - mean) * sc
    return np.minimum(np.maximum(x, np.float32(-clip)), np.float32(clip)).astype(np.float32)


def hidden_forward(x, w, b):
    """gb_epilogue_bf16<GEPI_TANH>: y = tanh(x w + b) before its rounding, and E"""
    z, s = affine(x, w, b)
    Ez = 2 * w.shape[0] * U * s
    y = np.tanh(z)
    return y, (1 - y * y) * Ez + 0.77 * Ez * Ez + TANH_ALLOW


def heads(h, w, b):
    """bf16_heads_kernel: the sum of the reduction ranges' partial products (+ the ranges' own additions), and E"""
    z, s = affine(h, w, b)
    return z, 2 * (w.shape[0] + 8) * U * s


def tanh_grad(dy, w, h):
    """gb_epilogue_bf16<GEPI_TANHGRAD>: y = (dy w^T) .* (1 - h^2) before its rounding, and E.  w [K_out][K_red] as it lies (dy [M][K_red])"""
    g, s = affine(dy, np.asarray(w, np.float64).T)
    h = np.asarray(h, np.float64)
    d = 1 - h * h
    y = g * d
    return y, np.abs(d) * (2 * w.shape[1] * U * s) + 4 * U * np.abs(y)


def column_sums(y, Ey, rows):
    """sums over `rows` fp32 values per column (bias gradients: M rows in the place of K, the unrounded values), and E"""
    y = np.asarray(y, np.float64)
    return y.sum(0), np.asarray(Ey, np.float64).sum(0) * np.ones(y.shape[1]) + 2 * rows * U * np.abs(y).sum(0)


def weight_grad(x, dy, extra_adds=0):
    """gemm_dw_bf16_kernel + assembly: x^T dy over the rows, and E (rows + the slabs' additions in the place of K)"""
    z, s = affine(np.asarray(x, np.float64).T, dy)
    return z, 2 * (x.shape[0] + extra_adds) * U * s


def head_sum_f32(parts):
    """head_sum(): the ranges' partial products added in range order in fp32 -- the device's own mu / v, bit for bit"""
    parts = np.asarray(parts, np.float32)
    s = parts[0].copy()
    for k in range(1, parts.shape[0]):
        s = (s + parts[k]).astype(np.float32)
    return s


def nlp_terms(mu, logstd, act):
    """float64 (z, sigma, ssq, nlp) and E_nlp, the bound on the kernels' fp32 neglogp (bf16_sample_kernel and bf16_loss_kernel take the same shape):
    z = (act - mu) / sigma: subtraction U, expf 2 ulp = 4 U, division U -> 6 U |z|, say 8; z^2: 2 * 8 + 1; the row sum is a 6-level tree behind at most
    two values per lane: 8 additions -> 0.5 ssq carries (17 + 8 + 1) U, say 32; HALF_LOG_2PI * A and the logstd sum: 1 + 8 additions, say 16."""
    mu = np.asarray(mu, np.float64); logstd = np.asarray(logstd, np.float64).reshape(1, -1); act = np.asarray(act, np.float64)
    sigma = np.exp(logstd)
    z = (act - mu) / sigma
    ssq = (z * z).sum(1)
    A = mu.shape[1]
    nlp = 0.5 * ssq + HALF_LOG_2PI * A + logstd.sum()
    E = U * (32 * 0.5 * ssq + 16 * (HALF_LOG_2PI * A + np.abs(logstd).sum()))
    return z, sigma, ssq, nlp, E


def act_epilogue(mu, logstd, noise):
    """bf16_sample_kernel from the kernel's own head sums `mu` (fp32): action = mu + sigma * eps and its bound (sigma: expf 2 ulp = 4 U, the product U,
    the sum U); neglogp is checked from the kernel's own ACTION (nlp_terms)"""
    mu = np.asarray(mu, np.float64); noise = np.asarray(noise, np.float64)
    sigma = np.exp(np.asarray(logstd, np.float64).reshape(1, -1))
    act = mu + sigma * noise
    return act, 6 * U * np.abs(sigma * noise) + 2 * U * np.abs(act)


def vf_loss_rows(v, R, vo, vcr, voff, gv):
    """vf_loss_row (ppo_kernels.hpp) in float64: (lossv, dv) per row; tests/test_value_clip.py states the three modes: vcr = cliprange (policy), the
    handle's own range (range), and voff = +inf (off: the clipped square becomes -inf, every row takes the unclipped side)"""
    dvo = v - vo
    vmin = np.minimum(dvo, vcr)
    vclip = vo + np.maximum(vmin, -vcr)
    e1, e2 = v - R, vclip - R
    with np.errstate(invalid="ignore"):
        s1, s2 = e1 * e1, e2 * e2 - voff
        lossv = np.maximum(s1, s2)
        selv = (s1 >= s2).astype(np.float64)
        passv = (vmin >= -vcr) * (dvo <= vcr) * 1.0
        dv = gv * selv * (2 * e1) + gv * (1 - selv) * (2 * e2) * passv
    return lossv, dv, np.abs(e1) + np.abs(e2)


def loss(mu, v, logstd, act, adv, ret, old_v, old_nlp, cr, vcr, voff, ent_coef, vf_coef):
    """bf16_loss_kernel in float64 from the kernel's own head sums (mu [n][A], v [n]).  Returns a dict: per-row gradients dmu / dl / dv with bounds,
    the five loss terms {pg, vf, entropy, approxkl, clipfrac} with bounds, the bias / logstd gradients (sums of the UNROUNDED values) with bounds."""
    n, A = mu.shape
    adv, ret, old_v, old_nlp, v = [np.asarray(x, np.float64) for x in (adv, ret, old_v, old_nlp, v)]
    g = float(np.float32(1.0) / np.float32(n))
    z, sigma, ssq, nlp, Enlp = nlp_terms(mu, logstd, act)
    ls = np.asarray(logstd, np.float64).reshape(1, -1)
    dk = nlp - old_nlp
    ratio = np.exp(-dk)
    lo, hi = 1.0 - cr, 1.0 + cr
    rmin = np.minimum(ratio, hi); rclip = np.maximum(rmin, lo)
    m1, m2 = -adv * ratio, -adv * rclip
    sel = (m1 >= m2) * 1.0
    pas = (rmin >= lo) * (ratio <= hi) * 1.0
    d_ratio = -adv * g * sel + -adv * g * (1 - sel) * pas
    d_nlp = -(d_ratio * ratio)
    dl = d_nlp[:, None] * (1 - z * z) - ent_coef * g
    dmu = d_nlp[:, None] * (-(z / sigma))
    # relative error of the fp32 ratio: the absolute error of its exponent (E_nlp, the subtraction) and expf's 2 ulp
    rr = Enlp + U * np.abs(dk) + 4 * U
    E_dmu = np.abs(dmu) * (rr[:, None] + 20 * U)                   # d_nlp: 3 products; z / sigma: 8 + 1 + 4; the last product
    E_dl = np.abs(d_nlp)[:, None] * ((rr[:, None] + 8 * U) * (1 + z * z) + 20 * U * z * z) + 4 * U * (np.abs(dl) + ent_coef * g)
    gv = float(np.float32(np.float32(vf_coef) * np.float32(0.5)) * np.float32(g))
    lossv, dv, esum = vf_loss_rows(v, ret, old_v, vcr, voff, gv)
    mag = np.abs(v) + np.abs(old_v) + np.abs(ret) + vcr            # every intermediate of vf_loss_row is at most this; at most 3 roundings precede e1 / e2
    E_dv = 6 * U * gv * mag + 8 * U * np.abs(dv)
    E_lossv = 2 * esum * 3 * U * mag + 2 * U * lossv
    pg = np.maximum(m1, m2)
    ent_row = (ls + HALF_LOG_2PIE).sum() * np.ones(n)
    cf = (np.abs(ratio - 1.0) > cr) * 1.0

    def mean_term(rows, E_rows, half=False):               # sum over the n rows in fp32 (n additions in the place of K), / n, (* 0.5)
        s = rows.sum() / n * (0.5 if half else 1.0)
        E = (E_rows.sum() + 2 * n * U * np.abs(rows).sum()) / n * (0.5 if half else 1.0)
        return s, E + 4 * U * abs(s)
    terms = [mean_term(pg, np.abs(pg) * (rr + 2 * U)), mean_term(lossv, E_lossv, True),
             mean_term(ent_row, 2 * (A + 8) * U * np.abs(ls + HALF_LOG_2PIE).sum() * np.ones(n)),
             mean_term(dk * dk, 2 * np.abs(dk) * (Enlp + U * np.abs(dk)) + U * dk * dk, True), mean_term(cf, np.zeros(n))]
    db_mu = column_sums(dmu, E_dmu, n)
    dlogstd = column_sums(dl, E_dl, n)
    db_v = (dv.sum(), E_dv.sum() + 2 * n * U * np.abs(dv).sum())
    return dict(dmu=dmu, E_dmu=E_dmu, dl=dl, dv=dv, E_dv=E_dv, nlp=nlp, E_nlp=Enlp, ratio=ratio, terms=terms, db_mu=db_mu, dlogstd=dlogstd, db_v=db_v)


def clip_adam(grad, theta, m, v, pow12, lr, max_norm, beta1, beta2, eps):
    """global-norm clip + Adam in float64 from the kernel's own assembled gradient (padded vectors).  Returns the norm, m', v', the step alpha and bounds:
    the sum of squares is a tree of at most ~50 additions of positive terms -> 51 U relative, its square root half of it + U, the clip factor two more
    roundings: the scaled gradient carries 36 U, say 40; m' = m + (gs - m)(1 - beta1): 40 U (|gs| + |m|); v': 80 U (gs^2 + |v|).  theta' is stated from the
    kernel's own m' and v' (theta_step): alpha (4 roundings), the product, sqrt, + eps, the quotient: 8 U of the step, and U of theta'."""
    grad = np.asarray(grad, np.float64); theta = np.asarray(theta, np.float64); m = np.asarray(m, np.float64); v = np.asarray(v, np.float64)
    norm = float(np.sqrt((grad * grad).sum()))
    scale = max_norm * min(1.0 / norm, 1.0 / max_norm)
    gs = grad * scale
    b1, b2 = float(np.float32(beta1)), float(np.float32(beta2))
    omb1, omb2 = float(np.float32(1.0) - np.float32(beta1)), float(np.float32(1.0) - np.float32(beta2))
    m1 = m + (gs - m) * omb1
    v1 = v + (gs * gs - v) * omb2
    alpha = float(np.float32(lr)) * np.sqrt(1.0 - float(pow12[1])) / (1.0 - float(pow12[0]))
    pow_after = np.array([np.float32(pow12[0]) * np.float32(b1), np.float32(pow12[1]) * np.float32(b2)], np.float32)
    return dict(norm=norm, E_norm=32 * U * norm, scale=scale, m=m1, E_m=40 * U * (np.abs(gs) + np.abs(m)), v=v1, E_v=80 * U * (gs * gs + np.abs(v)),
                alpha=alpha, pow_after=pow_after)


def theta_step(theta, m1, v1, alpha, eps):
    theta = np.asarray(theta, np.float64); m1 = np.asarray(m1, np.float64); v1 = np.asarray(v1, np.float64)
    step = m1 * alpha / (np.sqrt(v1) + float(np.float32(eps)))
    t = theta - step
    return t, 8 * U * np.abs(step) + U * np.abs(t)


# ---- the same stages in NumPy fp32 arithmetic (the emulation rules (2) and (3) take their caps from) -----------------------------------------------
def f32(x):
    return np.ascontiguousarray(x, dtype=np.float32)


K2 = np.float32(2.8853900817779268)        # 2 log2(e), the epilogue's constant


def emu_tanh_f32(acc, b):
    """the epilogue's tanh in fp32, in ITS form: 1 - 2 / (exp2(acc K2 + b K2) + 1).  The form matters: below |h| ~ 2^-7 the cancellation in 1 - 2 r leaves an
    ABSOLUTE error of ~1e-7 where bf16's spacing shrinks with |h|, so a few 1e-3 of a layer's elements land on the other side of a rounding boundary -- in
    any fp32 evaluation of this expression, the hardware's or NumPy's (a correctly rounded tanh, as np.tanh nearly is, shows none of them)."""
    acc, b = f32(acc), f32(b)
    arg = (acc.astype(np.float64) * np.float64(K2) + (b * K2).astype(np.float64)).astype(np.float32)      # fmaf(acc, K2, b * K2): one rounding
    e = np.exp2(arg, dtype=np.float32)
    r = np.float32(1.0) / (e + np.float32(1.0))
    return (np.float32(1.0) - np.float32(2.0) * r).astype(np.float32)                                      # fmaf(-2, r, 1): 2 r is exact


def emu_hidden_forward(x, w, b):
    return rne_bf16(emu_tanh_f32(f32(x) @ f32(w), b))


def emu_heads(h, w, b):
    return (f32(h) @ f32(w) + f32(b)).astype(np.float32)


def emu_tanh_grad_f32(dy, w, h):
    h = f32(h)
    return ((f32(dy) @ f32(w).T) * (np.float32(1.0) - h * h)).astype(np.float32)


def emu_weight_grad(x, dy):
    return (f32(x).T @ f32(dy)).astype(np.float32)


def emu_loss_grads_f32(mu, v, logstd, act, adv, ret, old_v, old_nlp, cr, vcr, voff, vf_coef):
    """bf16_loss_kernel's d mu and d v in NumPy fp32 arithmetic (every operation of the kernel's expression in fp32, NumPy's own summation order)"""
    F = np.float32
    mu, v, act, adv, ret, old_v, old_nlp = [f32(x) for x in (mu, v, act, adv, ret, old_v, old_nlp)]
    n, A = mu.shape
    ls = f32(logstd).reshape(1, -1)
    sigma = np.exp(ls)
    z = (act - mu) / sigma
    nlp = F(0.5) * (z * z).sum(1, dtype=F) + F(HALF_LOG_2PI) * F(A) + ls.sum(dtype=F)
    ratio = np.exp(old_nlp - nlp)
    lo, hi = F(1.0) - F(cr), F(1.0) + F(cr)
    rmin = np.minimum(ratio, hi); rclip = np.maximum(rmin, lo)
    g = F(1.0) / F(n)
    sel = ((-adv * ratio) >= (-adv * rclip)).astype(F)
    pas = (rmin >= lo).astype(F) * (ratio <= hi).astype(F)
    d_ratio = (-adv) * g * sel + (-adv) * g * (F(1.0) - sel) * pas
    d_nlp = -(d_ratio * ratio)
    dmu = d_nlp[:, None] * (-(z / sigma))
    gv = F(vf_coef) * F(0.5) * g
    dvo = v - old_v
    vmin = np.minimum(dvo, F(vcr)); vclip = old_v + np.maximum(vmin, F(-vcr))
    e1, e2 = v - ret, vclip - ret
    s1, s2 = e1 * e1, e2 * e2 - F(voff)
    selv = (s1 >= s2).astype(F)
    passv = (vmin >= F(-vcr)).astype(F) * (dvo <= F(vcr)).astype(F)
    dv = gv * selv * (F(2.0) * e1) + gv * (F(1.0) - selv) * (F(2.0) * e2) * passv
    return dmu.astype(F), dv.astype(F)


# ---- the padded parameter layout of a PPO_BF16 handle (build_layout in ppo_hip.hip: every dimension a multiple of 128, every tensor a multiple of 256 elements) --------
class Layout:
    PAD = 128

    def __init__(self, O, A, hidden):
        self.O, self.A, self.H = O, A, list(hidden)
        self.L = len(hidden)
        self.Kp0, self.Ap, self.Hp = ru(O, self.PAD), ru(A, self.PAD), [ru(h, self.PAD) for h in hidden]
        self.t, self.order = {}, []
        op = 0

        def add(name, rows, cols, prow, pcol):
            nonlocal op
            self.t[name] = (op, rows, cols, prow, pcol); self.order.append(name)
            op += ru(prow * pcol, 256)
        for l in range(self.L):
            inn, inp = (self.H[l - 1], self.Hp[l - 1]) if l else (O, self.Kp0)
            for tw in ("pi", "vf"):
                add("%s_fc%d/w" % (tw, l), inn, self.H[l], inp, self.Hp[l]); add("%s_fc%d/b" % (tw, l), self.H[l], 0, 1, self.Hp[l])
        add("vf/w", self.H[-1], 1, self.Hp[-1], self.Ap); add("vf/b", 1, 0, 1, self.Ap)
        add("pi/w", self.H[-1], A, self.Hp[-1], self.Ap); add("pi/b", A, 0, 1, self.Ap); add("pi/logstd", 1, A, 1, self.Ap)
        self.P_pad = op
        self.db_off, d = {}, 0                                     # bf.db_off: tower-major, then layer
        for tw in range(2):
            for l in range(self.L):
                self.db_off[(tw, l)] = d; d += self.Hp[l]
        self.n_dbias = d

    def mat(self, vec, name):
        """the padded [prow][pcol] view of a tensor of a padded vector"""
        off, rows, cols, prow, pcol = self.t[name]
        return vec[off:off + prow * pcol].reshape(prow, pcol)

    def dense(self, vec):
        out = []
        for name in self.order:
            off, rows, cols, prow, pcol = self.t[name]
            m = self.mat(vec, name)
            out.append((m[:rows, :cols] if cols else m[0, :rows]).ravel())
        return np.concatenate(out)

    def dense_mask(self):
        """True on the elements of the padded vector that are parameters"""
        idx = self.dense(np.arange(self.P_pad))
        m = np.zeros(self.P_pad, bool); m[idx] = True
        return m

    def params(self, vec):
        """{W[t][l], b[t][l], Wh[t], bh[t], logstd}: padded views of a padded vector (tower 0 = pi, 1 = vf)"""
        tw = ("pi", "vf")
        return dict(W=[[self.mat(vec, "%s_fc%d/w" % (t, l)) for l in range(self.L)] for t in tw],
                    b=[[self.mat(vec, "%s_fc%d/b" % (t, l))[0] for l in range(self.L)] for t in tw],
                    Wh=[self.mat(vec, "pi/w"), self.mat(vec, "vf/w")], bh=[self.mat(vec, "pi/b")[0], self.mat(vec, "vf/b")[0]],
                    logstd=self.mat(vec, "pi/logstd")[0])

    def dw_tiles(self):
        """the weight-gradient tile table of bf16_ensure_ws in its order (layer-major, the heads last): (tensor name, i0, j0, rows of the tile)"""
        bm = 256 if self.Kp0 % 256 == 0 and all(h % 256 == 0 for h in self.Hp) else 128
        tiles = []
        for l in range(self.L + 1):
            for t in ("pi", "vf"):
                name = "%s_fc%d/w" % (t, l) if l < self.L else "%s/w" % t
                _, _, _, prow, pcol = self.t[name]
                tiles += [(name, i, j, bm) for i in range(0, prow, bm) for j in range(0, pcol, 128)]
        return tiles

    def dw_split(self, Rp, max_split):
        """bf16_dw_split: (64-row stages per tile, stages per workgroup)"""
        nst = Rp // 64
        total = len(self.dw_tiles()) * nst
        per = max((total + 255) // 256, (nst + max_split - 3) // (max_split - 2))
        return nst, min(max(per, 1), nst)

    def slab_counts(self, Rp, max_split):
        """per element of the padded vector: how many slabs hold a partial sum of it (0 outside the weight matrices) -- the count bgr_chunk recomputes"""
        nst, per = self.dw_split(Rp, max_split)
        cnt = np.zeros(self.P_pad, np.int64)
        for tile, (name, i0, j0, bm) in enumerate(self.dw_tiles()):
            c = (tile * nst + nst - 1) // per - (tile * nst) // per + 1
            self.mat(cnt, name)[i0:i0 + bm, j0:j0 + 128] = c
        return cnt


def oracle_params(orc):
    """the fp32 oracle's weights in the shape Layout.params gives (no padding; the value head [H][1])"""
    d = orc.named()
    L = len(orc.hidden)
    return dict(W=[[d["%s_fc%d/w" % (t, l)] for l in range(L)] for t in ("pi", "vf")], b=[[d["%s_fc%d/b" % (t, l)] for l in range(L)] for t in ("pi", "vf")],
                Wh=[d["pi/w"], d["vf/w"]], bh=[d["pi/b"], d["vf/b"]], logstd=d["pi/logstd"].reshape(-1))


# ---- the stages chained end to end (rnd = identity: the fp32 oracle's mathematics; rnd = rne_bf16: the path's) ------------------------------------
def chain_forward(p, obs, rnd, A):
    """-> dict(x0, h[t][l], mu [n][A], v [n], Wb): every stage fed with the previous stage's (rounded) output"""
    L = len(p["W"][0])
    Wb = dict(W=[[r64(rnd, w) for w in p["W"][t]] for t in range(2)], Wh=[r64(rnd, w) for w in p["Wh"]])
    x0 = r64(rnd, obs)
    Kin = Wb["W"][0][0].shape[0]
    if x0.shape[1] < Kin:
        x0 = np.pad(x0, ((0, 0), (0, Kin - x0.shape[1])))
    h = [[], []]
    for t in range(2):
        x = x0
        for l in range(L):
            y, _ = hidden_forward(x, Wb["W"][t][l], p["b"][t][l])
            x = r64(rnd, y); h[t].append(x)
    mu = heads(h[0][-1], Wb["Wh"][0], p["bh"][0])[0][:, :A]
    v = heads(h[1][-1], Wb["Wh"][1], p["bh"][1])[0][:, 0]
    return dict(x0=x0, h=h, mu=mu, v=v, Wb=Wb)


def chain_train(p, mb, rnd, A, cr, vcr, voff, ent_coef, vf_coef):
    """forward, loss, backward and weight gradients chained -> (losses [5], {tensor name: gradient}, intermediates)"""
    L = len(p["W"][0])
    f = chain_forward(p, mb["obs"], rnd, A)
    ls = np.asarray(p["logstd"], np.float64)[:A]
    lo = loss(f["mu"], f["v"], ls, mb["actions"], mb["advs"], mb["returns"], mb["old_values"], mb["old_neglogp"], cr, vcr, voff, ent_coef, vf_coef)
    Wb = f["Wb"]
    n = f["mu"].shape[0]
    dhead = [np.zeros((n, Wb["Wh"][0].shape[1])), np.zeros((n, Wb["Wh"][1].shape[1]))]
    dhead[0][:, :A] = r64(rnd, lo["dmu"]); dhead[1][:, 0] = r64(rnd, lo["dv"])
    grads, dys = {}, [[None] * L, [None] * L]
    for t, tw in enumerate(("pi", "vf")):
        grads["%s/w" % tw] = weight_grad(f["h"][t][-1], dhead[t])[0]
        d = dhead[t]
        for l in range(L - 1, -1, -1):
            w = Wb["Wh"][t] if l == L - 1 else Wb["W"][t][l + 1]
            y, _ = tanh_grad(d, w, f["h"][t][l])
            grads["%s_fc%d/b" % (tw, l)] = y.sum(0)
            d = r64(rnd, y); dys[t][l] = d
            grads["%s_fc%d/w" % (tw, l)] = weight_grad(f["h"][t][l - 1] if l else f["x0"], d)[0]
    grads["pi/b"] = np.zeros(Wb["Wh"][0].shape[1]); grads["pi/b"][:A] = lo["db_mu"][0]
    grads["pi/logstd"] = lo["dlogstd"][0]
    grads["vf/b"] = np.array([lo["db_v"][0]])
    losses = np.array([t[0] for t in lo["terms"]])
    return losses, grads, dict(f=f, loss=lo, dhead=dhead, dy=dys)


def flat_grad(orc_tensors, grads):
    """the gradient dict in the dense flat order of `orc_tensors` [(name, off, shape)], every tensor cut to its dense shape"""
    out = []
    for name, _, shape in orc_tensors:
        g = np.asarray(grads[name])
        out.append((g[:shape[0], :shape[1]] if len(shape) == 2 and g.ndim == 2 else g.reshape(-1)[:int(np.prod(shape))]).ravel())
    return np.concatenate(out)


def cpu_chain_shares(p, mb, A, cr, ent_coef, vf_coef):
    """the CPU fp32 emulation of every GEMM stage on the inputs the rne_bf16 chain produces: {stage kind: largest mismatch share / relative L2 error}"""
    _, _, im = chain_train(p, mb, rne_bf16, A, cr, cr, 0.0, ent_coef, vf_coef)
    f, Wb = im["f"], im["f"]["Wb"]
    L = len(p["W"][0])
    out = {"hidden": 0.0, "dy": 0.0, "heads": 0.0, "dbias": 0.0, "dw": 0.0}
    for t in range(2):
        for l in range(L):
            x = f["h"][t][l - 1] if l else f["x0"]
            y, _ = hidden_forward(x, Wb["W"][t][l], p["b"][t][l])
            out["hidden"] = max(out["hidden"], mismatch_share(emu_hidden_forward(x, Wb["W"][t][l], p["b"][t][l]), y))
            d = im["dy"][t][l + 1] if l < L - 1 else im["dhead"][t]
            w = Wb["W"][t][l + 1] if l < L - 1 else Wb["Wh"][t]
            y, _ = tanh_grad(d, w, f["h"][t][l])
            e = emu_tanh_grad_f32(d, w, f["h"][t][l])
            if np.abs(y).max() > 0:
                out["dy"] = max(out["dy"], mismatch_share(rne_bf16(e), y))
                out["dbias"] = max(out["dbias"], rel_l2(e.sum(0, dtype=np.float32), y.sum(0)))
                out["dw"] = max(out["dw"], rel_l2(emu_weight_grad(x, im["dy"][t][l]), weight_grad(x, im["dy"][t][l])[0]))
        z, _ = heads(f["h"][t][-1], Wb["Wh"][t], p["bh"][t])
        cols = slice(0, A) if t == 0 else slice(0, 1)
        out["heads"] = max(out["heads"], rel_l2(emu_heads(f["h"][t][-1], Wb["Wh"][t], p["bh"][t])[:, cols], z[:, cols]))
    ls = np.asarray(p["logstd"], np.float64)[:A]
    dmu32, _ = emu_loss_grads_f32(f["mu"].astype(np.float32), f["v"].astype(np.float32), ls, mb["actions"], mb["advs"], mb["returns"], mb["old_values"], mb["old_neglogp"],
                                  cr, cr, 0.0, vf_coef)
    out["dhead"] = mismatch_share(rne_bf16(dmu32), im["loss"]["dmu"])
    return out
