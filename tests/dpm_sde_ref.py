"""The stochastic DPM-Solver++(2M) restated in float64 numpy, with no import from the product (``dpm_ref`` supplies the schedule, the
grids and the Gaussian denoiser): the coefficient rows for a given eta, one update, the whole loop on a list of noise arrays, the float32
rounding budget of one update and of a loop, and the closed-form final variance of the loop on Gaussian data.

A row is dpm_ref's seven fields plus sigma_n:  (s1m, sqrt_a, c_x, c_0, c_1, q_sqrt_a, q_s1m, sigma_n) with
    c_x = (sigma_tgt / sigma_cur) * exp(-eta*h),   E = -alpha_tgt * expm1(-(1 + eta)*h),   c_0 = E*(1 + 1/(2r)),   c_1 = -E/(2r),
    sigma_n = sigma_tgt * sqrt(-expm1(-2*eta*h))."""
import numpy as np

import dpm_ref
from dpm_ref import U, _abs, _f64

FIELDS = dpm_ref.FIELDS + ("sigma_n",)


def rows(ab, ts, t_start=None, order=2, lower_order_final=True, eta=1.0, flip_history=False):
    """float64 [t_start + 1, 8] rows of a loop i = t_start .. 0 over the grid ts.  flip_history: the (wrong) form with the sign of the
    1/(2r) terms flipped, for the comparison of property 3."""
    ab = np.asarray(ab, np.float64)
    t_start = len(ts) - 1 if t_start is None else t_start
    ts = np.asarray(ts)[: t_start + 1]
    n = len(ts)
    out, h = np.zeros((n, 8)), np.zeros(n)
    level = lambda i: (ab[ts[i]], ab[ts[i - 1]] if i > 0 else ab[0])
    for i in range(n):
        cur, tgt = level(i)
        h[i] = dpm_ref.lam(tgt) - dpm_ref.lam(cur)
    for i in range(n):
        cur, tgt = level(i)
        first = i == n - 1 or order == 1 or h[i] == 0 or h[i + 1] == 0 or (i == 0 and lower_order_final and n < 15)
        E = -np.sqrt(tgt) * np.expm1(-(1 + eta) * h[i])
        inv2r = 0.0 if first else 1.0 / (2.0 * (h[i + 1] / h[i]))
        if flip_history:
            inv2r = -inv2r
        out[i] = (np.sqrt(1 - cur), np.sqrt(cur), np.sqrt(1 - tgt) / np.sqrt(1 - cur) * np.exp(-eta * h[i]), E * (1 + inv2r), -E * inv2r,
                  np.sqrt(cur), np.sqrt(1 - cur), np.sqrt(1 - tgt) * np.sqrt(max(0.0, -np.expm1(-2 * eta * h[i]))))
    return out


def levels(ab, ts):
    """(alpha_bar of the current, of the target time step) per grid index."""
    ab, ts = np.asarray(ab, np.float64), np.asarray(ts)
    return ab[ts], np.concatenate([ab[:1], ab[ts[:-1]]])


def update(row, x, eps, x0_prev=None, noise=None, orig=None, orig_noise=None, mask=None):
    """(x_out, x0) of one step in float64: the history only when c_1 != 0, the noise only when sigma_n != 0, the noise BEFORE the blend."""
    s1m, sqrt_a, c_x, c_0, c_1, q_a, q_s, sigma_n = (float(v) for v in row)
    x, eps = _f64(x), _f64(eps)
    x0 = (x - s1m * eps) / sqrt_a
    out = c_x * x + c_0 * x0
    if c_1 != 0:
        out = out + c_1 * _f64(x0_prev)
    if sigma_n != 0:
        out = out + sigma_n * _f64(noise)
    if orig is not None:
        m = _f64(mask)
        out = (q_a * _f64(orig) + q_s * _f64(orig_noise)) * m + out * (1 - m)
    return out, x0


def budget(row, x, eps, x0_prev=None, noise=None, orig=None, orig_noise=None, mask=None):
    """(bound on |x_out(float32) - x_out(float64)|, the same for x0) per element by dpm_ref.budget's counting: the roundings counted beside
    the kernel (3 for x0; 6 / 8 for a first / second order step, 2 more with the noise term - its product and its addition -, 7 more with
    the known region) times 2^-24 times the sum of the magnitudes of the terms added up, |sigma_n*z| among them.  No fitted constant; the
    same precondition |c_0| <= 4*sqrt_a*|c_x| (see dpm_ref.budget) is asserted."""
    s1m, sqrt_a, c_x, c_0, c_1, q_a, q_s, sigma_n = (abs(float(v)) for v in row)
    assert c_0 <= 4 * sqrt_a * c_x, "budget(): |c_0| <= 4*sqrt_a*|c_x| does not hold for this row"
    x0 = update(row, x, eps)[1]
    b0 = 3 * U * (_abs(x) / sqrt_a + s1m * _abs(eps) / sqrt_a)
    terms, n = c_x * _abs(x) + c_0 * np.abs(x0), 6
    if c_1 != 0:
        terms, n = terms + c_1 * _abs(x0_prev), 8
    if sigma_n != 0:
        terms, n = terms + sigma_n * _abs(noise), n + 2
    if orig is not None:
        terms, n = terms * np.abs(1 - _f64(mask)) + (q_a * _abs(orig) + q_s * _abs(orig_noise)) * _abs(mask), n + 7
    return n * U * terms, b0


def loop(R, x, eps_of, noises, known=None, ancestors=None):
    """The loop over the rows R (index len(R) - 1 down to 0) in float64.  noises[k]: the noise array of the k-th step of the loop.
    ancestors: {k: index array over the leading axis} - before the update of step k, x, eps and the history move to these rows (a
    steering event; on step 0 there is no history yet)."""
    x, x0p = _f64(x), None
    kw = {} if known is None else dict(orig=known[0], orig_noise=known[1], mask=known[2])
    for k, i in enumerate(range(len(R) - 1, -1, -1)):
        assert R[i][4] == 0 or x0p is not None
        e = eps_of(i, x)
        if ancestors is not None and k in ancestors:
            a = np.asarray(ancestors[k])
            x, e, x0p = x[a], e[a], (None if x0p is None else x0p[a])
        x, x0p = update(R[i], x, e, x0p, noises[k], **kw)
    return x


def loop_gauss_with_budget(R, gains, x, noises, ancestors=None, history_moves=True):
    """dpm_ref.loop_gauss_with_budget for the stochastic loop fed GIVEN noise arrays (the float32 run reads the same values, so the noise
    carries no error of its own): the denoiser is eps = gains[i] * x, one float32 product.  The step is linear in x and the history, so an
    incoming error is carried by the same factors as there; the noise term only adds its two roundings, which budget() counts.  A steering
    event (ancestors, as in loop) moves the error bounds with the rows; history_moves=False is the (wrong) loop that leaves the history
    where it was.  Returns (x_end, bound)."""
    x = _f64(x)
    ex, e0, x0p = np.zeros_like(x), np.zeros_like(x), None
    for k, i in enumerate(range(len(R) - 1, -1, -1)):
        s1m, sqrt_a, c_x, c_0, c_1 = (float(v) for v in R[i][:5])
        g = float(gains[i])
        if ancestors is not None and k in ancestors:
            a = np.asarray(ancestors[k])
            x, ex = x[a], ex[a]
            if history_moves and x0p is not None:
                e0, x0p = e0[a], x0p[a]
        eps = g * x
        rho = U * np.abs(eps)
        kappa = (1 - s1m * g) / sqrt_a
        bx, b0 = budget(R[i], x, eps, x0p, noises[k])
        ex, e0 = (abs(c_x + c_0 * kappa) * ex + abs(c_1) * e0 + abs(c_0) * (s1m / sqrt_a) * rho + bx,
                  abs(kappa) * ex + (s1m / sqrt_a) * rho + b0)
        x, x0p = update(R[i], x, eps, x0p, noises[k])
    return x, ex


def gauss_cov(R, gains, v_T):
    """The final variance of the loop on the linear denoiser eps = gains[i]*x, in closed form: x0 = kappa*x with kappa = (1 - s1m*g)/sqrt_a,
    so (x, x0_prev) -> ((c_x + c_0*kappa)*x + c_1*x0_prev + sigma_n*z, kappa*x) is linear; the 2x2 covariance of (x, x0_prev) goes through
    that map and sigma_n^2 is added to the variance of x.  v_T: the variance x starts with."""
    P = np.array([[float(v_T), 0.0], [0.0, 0.0]])
    for i in range(len(R) - 1, -1, -1):
        s1m, sqrt_a, c_x, c_0, c_1 = (float(v) for v in R[i][:5])
        kappa = (1 - s1m * float(gains[i])) / sqrt_a
        A = np.array([[c_x + c_0 * kappa, c_1], [kappa, 0.0]])
        P = A @ P @ A.T
        P[0, 0] += float(R[i][7]) ** 2
    return float(P[0, 0])


def var_err(ab, n_steps, s, eta=1.0, kind="logsnr", **kw):
    """Relative error of the loop's final variance against the exact ab_0*s^2 + 1 - ab_0, from a start on the marginal of the top time step."""
    ts = dpm_ref.grid(ab, n_steps, kind)
    R = rows(ab, ts, eta=eta, **kw)
    v = lambda t: ab[t] * s * s + 1 - ab[t]
    got = gauss_cov(R, [dpm_ref.gauss_gain(ab, t, s) for t in ts], v(ts[-1]))
    return got / v(0) - 1.0
