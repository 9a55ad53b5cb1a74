"""Exact DDIM inversion restated in float64 numpy, with no import from the product: the coefficient rows of the upward step, one
fixed-point iterate, its float32 rounding budget, the DDIM step (eta = 0) it inverts with a budget of its own, the upward loop and the
round trip on the closed-form Gaussian denoiser of ``dpm_ref`` with accumulated bounds on how far a float32 run can be from them.

Notation: ab = alpha_bar; grid index i counts up with the time step.  The DDIM step at index i goes from level a = ab[ts[i]] DOWN to
ap = ab[ts[i - 1]] (ab[0] at i = 0) and evaluates the denoiser at time step ts[i]:
    F(x) = sqrt(ap) * (x - sqrt(1 - a) * eps(x)) / sqrt(a) + sqrt(1 - ap) * eps(x) = (x - c_e * eps(x)) / c_y
    c_y = sqrt(a / ap),  c_e = sqrt(1 - a) - sqrt(a * (1 - ap) / ap)
The upward step looks for the x with F(x) = y by K iterates x <- c_y*y + c_e*eps(x) from x = y; F(x_K) - y = (x_K - x_K+1) / c_y."""
import numpy as np

import dpm_ref

U = dpm_ref.U           # unit roundoff of float32
FIELDS = ("c_y", "c_e")


def _f64(v):
    return np.asarray(v, np.float64)


def _abs(v):
    return np.abs(_f64(v))


def levels(ab, ts):
    """(a, ap) per grid index, float64."""
    ab, ts = _f64(ab), np.asarray(ts)
    return ab[ts], np.concatenate([ab[0:1], ab[ts[:-1]]])


# ---------------------------------------------------------------------------------------------- coefficients
def rows(ab, ts):
    """float64 [len(ts), 2]: (c_y, c_e) of the upward step at every grid index; a repeated time step is the identity (1, 0)."""
    a, ap = levels(ab, ts)
    out = np.stack([np.sqrt(a / ap), np.sqrt(1 - a) - np.sqrt(a * (1 - ap) / ap)], axis=1)
    out[a == ap] = (1.0, 0.0)
    return out


def ddim_rows(ab, ts):
    """float64 [len(ts), 4]: (s1m, sqrt_a, sqrt_aprev, dir_coef) of the eta = 0 DDIM step at every grid index."""
    a, ap = levels(ab, ts)
    return np.stack([np.sqrt(1 - a), np.sqrt(a), np.sqrt(ap), np.sqrt(1 - ap)], axis=1)


# ---------------------------------------------------------------------------------------------- one iterate, one DDIM step
def update(row, y, eps):
    """One iterate in float64: c_y*y + c_e*eps."""
    return float(row[0]) * _f64(y) + float(row[1]) * _f64(eps)


def budget(row, y, eps):
    """Bound on |x_out(float32) - x_out(float64)| per element for the kernel's individually rounded float32 operations on these float32
    inputs.  Counted beside the kernel (csrc/sampler_steps.hip): mul (c_y*y), mul (c_e*eps), add = 3 roundings, times 2^-24, times the sum
    of the magnitudes of the terms that are added up, |c_y*y| + |c_e*eps|.  Nothing cancels before the sum, so no side condition; no
    fitted constant."""
    return 3 * U * (abs(float(row[0])) * _abs(y) + abs(float(row[1])) * _abs(eps))


def forward(drow, x, eps):
    """The DDIM step F in float64, in pf_ddim_step's operation order."""
    s1m, sqrt_a, sqrt_ap, dirc = (float(v) for v in drow[:4])
    return sqrt_ap * ((_f64(x) - s1m * _f64(eps)) / sqrt_a) + dirc * _f64(eps)


def forward_budget(drow, x, eps):
    """The same for pf_ddim_step (sigma = 0, no known region), rounding by rounding: t1 = s1m*eps, t2 = x - t1, p0 = t2/sqrt_a,
    t3 = sqrt_aprev*p0, t4 = dir_coef*eps, out = t3 + t4 - 6 roundings.  The one of t1 reaches the result times sqrt_aprev/sqrt_a; those of
    t2, p0, t3 and out are each at most u*|sqrt_aprev*p0| there (|t2| = sqrt_a*|p0|), those of t4 and out u*|dir_coef*eps|:
        u * ((sqrt_aprev/sqrt_a)*|s1m*eps| + 4*|sqrt_aprev*p0| + 2*|dir_coef*eps|)."""
    s1m, sqrt_a, sqrt_ap, dirc = (abs(float(v)) for v in drow[:4])
    p0 = (_f64(x) - float(drow[0]) * _f64(eps)) / float(drow[1])
    return U * ((sqrt_ap / sqrt_a) * s1m * _abs(eps) + 4 * sqrt_ap * np.abs(p0) + 2 * dirc * _abs(eps))


# ---------------------------------------------------------------------------------------------- loops, any denoiser
def invert_loop(R, x0, eps_of, K, t_end=None, keep=None):
    """The upward loop over the rows R, indices 0 .. t_end, K iterates per step from x = y, in float64; eps_of(i, x) is the denoiser at
    grid index i.  keep (a list): receives [step][k] iterates."""
    y = _f64(x0)
    t_end = len(R) - 1 if t_end is None else t_end
    for i in range(t_end + 1):
        x = y
        if keep is not None:
            keep.append([])
        for _ in range(K):
            x = update(R[i], y, eps_of(i, x))
            if keep is not None:
                keep[-1].append(x)
        y = x
    return y


def paint_loop(D, x, eps_of, t_start=None):
    """DDIM with eta = 0 over the rows D, indices t_start .. 0, in float64."""
    x = _f64(x)
    t_start = len(D) - 1 if t_start is None else t_start
    for i in range(t_start, -1, -1):
        x = forward(D[i], x, eps_of(i, x))
    return x


# ---------------------------------------------------------------------------------------------- the analytic case
def contraction(R, gains):
    """|c_e * g| per grid index: the factor by which one iterate shrinks the distance to the fixed point when eps = g * x."""
    return np.abs(_f64(R)[:, 1] * _f64(gains))


def invert_gauss_with_budget(R, gains, x0, K, t_end=None):
    """The upward loop on the denoiser eps = gains[i] * x in float64, with a bound on how far a float32 run - the kernel's operations, and
    ONE float32 product for eps - can be from it at the end.  Per element, with ey the bound on the error of y entering a step (it stays
    for all K iterates), ek the one of the iterate x_k (e_0 = ey, the iteration starts from y) and rho = u*|g*x_k| the rounding of eps:
        e_k+1 <= |c_y|*ey + |c_e|*(|g|*ek + rho) + budget(row, y, eps)
    (an iterate is linear in y and in eps, so incoming errors are carried by exactly these factors).  First order in u: the budgets are
    evaluated on the float64 values.  Returns (x_end, bound, residuals [steps, K]) - residuals[i, k] = |x_k+1 - x_k|_2 / |x_k+1|_2 over all
    elements."""
    y = _f64(x0)
    t_end = len(R) - 1 if t_end is None else t_end
    ey = np.zeros_like(y)
    res = np.zeros((t_end + 1, K))
    for i in range(t_end + 1):
        c_y, c_e, g = float(R[i][0]), float(R[i][1]), float(gains[i])
        x, ek = y, ey
        for k in range(K):
            eps = g * x
            rho = U * np.abs(eps)
            ek = abs(c_y) * ey + abs(c_e) * (abs(g) * ek + rho) + budget(R[i], y, eps)
            nxt = update(R[i], y, eps)
            res[i, k] = np.sqrt(np.sum((nxt - x) ** 2) / np.sum(nxt ** 2))
            x = nxt
        y, ey = x, ek
    return y, ey, res


def paint_gauss_with_budget(D, gains, x, e_in=None, t_start=None):
    """DDIM (eta = 0) down the rows D on eps = gains[i] * x in float64, with the bound carried on from e_in (the bound on x as it enters):
        e' <= |sqrt_aprev*(1 - s1m*g)/sqrt_a + dir_coef*g| * e + (sqrt_aprev*s1m/sqrt_a + dir_coef) * rho + forward_budget
    Returns (x_end, bound)."""
    x = _f64(x)
    e = np.zeros_like(x) if e_in is None else _f64(e_in)
    t_start = len(D) - 1 if t_start is None else t_start
    for i in range(t_start, -1, -1):
        s1m, sqrt_a, sqrt_ap, dirc = (float(v) for v in D[i][:4])
        g = float(gains[i])
        eps = g * x
        rho = U * np.abs(eps)
        e = abs(sqrt_ap * (1 - s1m * g) / sqrt_a + dirc * g) * e + (sqrt_ap * s1m / sqrt_a + dirc) * rho + forward_budget(D[i], x, eps)
        x = forward(D[i], x, eps)
    return x, e


def roundtrip_err(ab, ts, s, K):
    """max |paint(invert(x0)) - x0| / max |x0| in float64 on the Gaussian denoiser N(0, s^2), exact float64 rows, x0 = 1."""
    gains = dpm_ref.gauss_gain(ab, np.asarray(ts), s)
    x0 = np.ones(1)
    x = invert_loop(rows(ab, ts), x0, lambda i, v: gains[i] * v, K)
    back = paint_loop(ddim_rows(ab, ts), x, lambda i, v: gains[i] * v)
    return dpm_ref.rel_err(back, x0)
