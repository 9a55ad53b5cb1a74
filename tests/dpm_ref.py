"""DPM-Solver++(2M) restated in float64 numpy, with no import from the product: the time-step grids, the coefficient rows, one update
(with the known-region blend), the whole loop, DDIM with eta = 0 for comparison, the closed-form optimal denoiser for Gaussian data with
the exact solution of its probability-flow ODE, and the float32 rounding budgets the GPU tests hold the kernel to.

Notation: ab = alpha_bar, alpha = sqrt(ab), sigma = sqrt(1 - ab), lambda = log(alpha / sigma).  Grid index i counts up with the time
step; step i goes from time_steps[i] to time_steps[i - 1], and to time step 0 at i = 0.  A coefficient row is
(s1m, sqrt_a, c_x, c_0, c_1, q_sqrt_a, q_s1m)."""
import numpy as np

U = 2.0 ** -24          # unit roundoff of float32 (round to nearest)
FIELDS = ("s1m", "sqrt_a", "c_x", "c_0", "c_1", "q_sqrt_a", "q_s1m")


def alpha_bar(n_steps=1000, linear_start=0.00085, linear_end=0.012):
    """The project's schedule, held in float32 as the models hold it, returned as float64."""
    beta = np.linspace(linear_start ** 0.5, linear_end ** 0.5, n_steps, dtype=np.float64) ** 2
    return np.cumprod(1.0 - beta).astype(np.float32).astype(np.float64)


def lam(a):
    return 0.5 * np.log(a / (1.0 - a))


# ---------------------------------------------------------------------------------------------- grids
def grid_uniform(n, n_steps):
    return np.arange(0, n, n // n_steps) + 1


def grid_quad(n, n_steps):
    return (np.linspace(0, np.sqrt(n * 0.8), n_steps) ** 2).astype(int) + 1


def grid_logsnr(ab, n_steps):
    n, l = len(ab), lam(np.asarray(ab, np.float64))
    ts = sorted({int(np.argmin(np.abs(l - t))) for t in np.linspace(l[n - 1], l[1], n_steps)} - {0})
    return np.asarray(ts, dtype=np.int64)


def grid(ab, n_steps, kind):
    return {"uniform": lambda: grid_uniform(len(ab), n_steps), "quad": lambda: grid_quad(len(ab), n_steps),
            "logsnr": lambda: grid_logsnr(ab, n_steps)}[kind]()


# ---------------------------------------------------------------------------------------------- coefficients
def rows(ab, ts, t_start=None, order=2, lower_order_final=True):
    """float64 [t_start + 1, 7] rows of a loop i = t_start .. 0 over the grid ts."""
    ab = np.asarray(ab, np.float64)
    t_start = len(ts) - 1 if t_start is None else t_start
    ts = np.asarray(ts)[: t_start + 1]
    n = len(ts)
    out = np.zeros((n, 7))
    h = np.zeros(n)
    for i in range(n):
        cur, tgt = ab[ts[i]], (ab[ts[i - 1]] if i > 0 else ab[0])
        h[i] = lam(tgt) - lam(cur)
    for i in range(n):
        cur, tgt = ab[ts[i]], (ab[ts[i - 1]] if i > 0 else ab[0])
        first = i == n - 1 or order == 1 or h[i] == 0 or h[i + 1] == 0 or (i == 0 and lower_order_final and n < 15)
        phi = -np.sqrt(tgt) * np.expm1(-h[i])
        inv2r = 0.0 if first else 1.0 / (2.0 * (h[i + 1] / h[i]))
        out[i] = (np.sqrt(1 - cur), np.sqrt(cur), np.sqrt(1 - tgt) / np.sqrt(1 - cur), phi * (1 + inv2r), -phi * inv2r,
                  np.sqrt(cur), np.sqrt(1 - cur))
    return out


# ---------------------------------------------------------------------------------------------- one update
def update(row, x, eps, x0_prev=None, orig=None, orig_noise=None, mask=None):
    """(x_out, x0) of one step in float64; x0_prev takes part only when c_1 != 0."""
    s1m, sqrt_a, c_x, c_0, c_1, q_a, q_s = (float(v) for v in row)
    x, eps = np.asarray(x, np.float64), np.asarray(eps, np.float64)
    x0 = (x - s1m * eps) / sqrt_a
    out = c_x * x + c_0 * x0
    if c_1 != 0:
        out = out + c_1 * np.asarray(x0_prev, np.float64)
    if orig is not None:
        m = np.asarray(mask, np.float64)
        out = (q_a * np.asarray(orig, np.float64) + q_s * np.asarray(orig_noise, np.float64)) * m + out * (1 - m)
    return out, x0


def budget(row, x, eps, x0_prev=None, orig=None, orig_noise=None, mask=None):
    """(bound on |x_out(float32) - x_out(float64)|, the same for x0) per element, for the kernel's individually rounded float32 operations on
    these float32 inputs: the number of roundings on the way to the result (counted beside the kernel in csrc/sampler_steps.hip: 3 for x0,
    6 for a first-order step, 8 for a second-order one, 7 more with the known-region blend) times 2^-24 times the sum of the magnitudes of
    the terms that are added up.  No fitted constant.

    x0 = (x - s1m*eps)/sqrt_a: its terms are x/sqrt_a and s1m*eps/sqrt_a.
    x_out: |c_x*x| + |c_0*x0| + |c_1*x0_prev|, and with a known region that sum times |1 - m| plus (|q_sqrt_a*orig| + |q_s1m*orig_noise|)*|m|.
    One thing this sum does not see is cancellation INSIDE x0: the rounding of s1m*eps, u*|s1m*eps|/sqrt_a, reaches x_out multiplied by
    c_0 however small x0 itself comes out.  It is covered by the count whenever |c_0| <= 4*sqrt_a*|c_x| - then
    |c_0|*|s1m*eps|/sqrt_a <= |c_0|*(|x0| + |x|/sqrt_a) <= |c_0*x0| + 4*|c_x*x|, and a first-order step spends only 2 of its 6 roundings on
    c_x*x and 4 on c_0*x0, a second-order one 3 and 5 of 8 - which is asserted here, and holds on the schedule's rows for any grid of about
    ten steps or more (|c_0|/(sqrt_a*c_x) is about (exp(h) - 1)*1.5/c_x)."""
    s1m, sqrt_a, c_x, c_0, c_1, q_a, q_s = (abs(float(v)) for v in row)
    assert c_0 <= 4 * sqrt_a * c_x, "budget(): |c_0| <= 4*sqrt_a*|c_x| does not hold for this row"
    x0 = update(row, x, eps)[1]
    b0 = 3 * U * (_abs(x) / sqrt_a + s1m * _abs(eps) / sqrt_a)
    terms, n = c_x * _abs(x) + c_0 * np.abs(x0), 6
    if c_1 != 0:
        terms, n = terms + c_1 * _abs(x0_prev), 8
    if orig is not None:
        terms, n = terms * np.abs(1 - _f64(mask)) + (q_a * _abs(orig) + q_s * _abs(orig_noise)) * _abs(mask), n + 7
    return n * U * terms, b0


def _f64(v):
    return np.asarray(v, np.float64)


def _abs(v):
    return np.abs(_f64(v))


# ---------------------------------------------------------------------------------------------- loops
def loop(R, x, eps_of, known=None):
    """The 2M loop over the rows R (index len(R) - 1 down to 0) in float64; eps_of(i, x) is the denoiser at grid index i;
    known = (orig, orig_noise, mask) or None.  The history starts empty: the top row is first order."""
    x, x0p = _f64(x), None
    kw = {} if known is None else dict(orig=known[0], orig_noise=known[1], mask=known[2])
    for i in range(len(R) - 1, -1, -1):
        assert R[i][4] == 0 or x0p is not None
        x, x0p = update(R[i], x, eps_of(i, x), x0p, **kw)
    return x


def ddim_loop(ab, ts, x, eps_of):
    """DDIM with eta = 0 over the grid ts, in float64: x_prev = sqrt(ab_prev)*x0 + sqrt(1 - ab_prev)*eps."""
    ab, x = _f64(ab), _f64(x)
    for i in range(len(ts) - 1, -1, -1):
        cur, prev = ab[ts[i]], (ab[ts[i - 1]] if i > 0 else ab[0])
        e = eps_of(i, x)
        x = np.sqrt(prev) * (x - np.sqrt(1 - cur) * e) / np.sqrt(cur) + np.sqrt(1 - prev) * e
    return x


# ---------------------------------------------------------------------------------------------- the analytic case
def gauss_gain(ab, t, s):
    """The optimal denoiser for data ~ N(0, s^2): x_t ~ N(0, v_t) with v_t = ab_t*s^2 + 1 - ab_t, and E[noise | x_t] = gain * x_t."""
    a = _f64(ab)[t]
    return np.sqrt(1 - a) / (a * s * s + 1 - a)


def gauss_exact(ab, t_from, s, x):
    """The probability-flow ODE's exact solution from time step t_from down to time step 0: x scales with the standard deviation."""
    v = lambda t: _f64(ab)[t] * s * s + 1 - _f64(ab)[t]
    return _f64(x) * np.sqrt(v(0) / v(t_from))


def rel_err(x_num, x_exact):
    return float(np.abs(_f64(x_num) - x_exact).max() / np.abs(x_exact).max())


def err_2m(ab, n_steps, s, kind="logsnr"):
    ts = grid(ab, n_steps, kind)
    x = np.ones(1)
    return rel_err(loop(rows(ab, ts), x, lambda i, v: gauss_gain(ab, ts[i], s) * v), gauss_exact(ab, ts[-1], s, x))


def err_ddim(ab, n_steps, s, kind="uniform"):
    ts = grid(ab, n_steps, kind)
    x = np.ones(1)
    return rel_err(ddim_loop(ab, ts, x, lambda i, v: gauss_gain(ab, ts[i], s) * v), gauss_exact(ab, ts[-1], s, x))


def loop_gauss_with_budget(R, gains, x):
    """The 2M loop on a denoiser eps = gains[i] * x (elementwise), in float64, with a bound on how far a float32 run - the kernel's
    operations, and ONE float32 product for eps - can be from it at the end.  Per element, with ex / e0 the bounds on the errors of x and
    of the history entering a step, kappa = (1 - s1m*g)/sqrt_a (so that x0 = kappa*x) and rho <= u*|eps| the rounding of eps:
        x0 error  <= |kappa|*ex + (s1m/sqrt_a)*rho + budget_x0
        x error   <= |c_x + c_0*kappa|*ex + |c_1|*e0 + |c_0|*(s1m/sqrt_a)*rho + budget_x
    (the step is linear in x and in the history, so an incoming error is carried by exactly these factors; budget_* are budget()'s).
    First order in u: the budgets are evaluated on the float64 values.  Returns (x_end, bound)."""
    x = _f64(x)
    ex, e0, x0p = np.zeros_like(x), np.zeros_like(x), None
    for i in range(len(R) - 1, -1, -1):
        s1m, sqrt_a, c_x, c_0, c_1 = (float(v) for v in R[i][:5])
        g = float(gains[i])
        eps = g * x
        rho = U * np.abs(eps)
        kappa = (1 - s1m * g) / sqrt_a
        bx, b0 = budget(R[i], x, eps, x0p)
        ex, e0 = (abs(c_x + c_0 * kappa) * ex + abs(c_1) * e0 + abs(c_0) * (s1m / sqrt_a) * rho + bx,
                  abs(kappa) * ex + (s1m / sqrt_a) * rho + b0)
        x, x0p = update(R[i], x, eps, x0p)
    return x, ex
