"""numpy restatement of the steering kernels (include/pfhip.h: ``pf_x0_predict``, ``pf_steer_resample``, ``pf_rows_gather``), written from
the definition and from nothing of the kernels: float64 scalars for the resampling rule (numpy rounds every operation on its own), Python
integers for the Philox word behind ``u`` (``tests/noise_matrix.py``), float32 arrays for the predicted x0, and the steered loop written
by hand on top of the samplers' own single-step calls."""
import math

import numpy as np

import noise_matrix

F = np.float32
D = np.float64
MAX_N = 256
KEY_TAG = 0x53544552
M32 = 0xFFFFFFFF
# planted defects of resample(): each must be caught by tests/test_steer_host.py
DEFECTS = ("tree_sum", "strict_ess", "u53", "base_on_keep")


def u_word(seed, g, event):
    """The first output word of Philox4x32-10 with counter (g lo, g hi, event lo, event hi) and key (seed lo, seed hi ^ KEY_TAG)."""
    ctr = (g & M32, (g >> 32) & M32, event & M32, (event >> 32) & M32)
    return noise_matrix.philox4x32(ctr, (seed & M32, ((seed >> 32) & M32) ^ KEY_TAG))[0]


def u_of(seed, g, event):
    return D(u_word(seed, g, event)) * D(2.0 ** -32)


def weights_of(reward, base, lam):
    """Rules 1 and 2 for one group: float64 ``[n]`` and whether any particle has a finite weight."""
    reward, base = np.asarray(reward, D), np.asarray(base, D)
    with np.errstate(all="ignore"):
        lw = D(lam) * (reward - base)
        ok = np.isfinite(reward) & np.isfinite(lw)
        if not ok.any():
            return np.zeros(reward.size, D), False
        m = lw[ok].max()
        return np.where(ok, np.exp(np.where(ok, lw - m, D(0.0))), D(0.0)), True


def serial_sums(w, defect=None):
    """``(S, Q, c)``: the sums added serially in index order and the running sum of S."""
    if defect == "tree_sum":
        v, q = list(w), [D(x) * D(x) for x in w]
        while len(v) > 1:
            v = [v[i] + v[i + 1] if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
            q = [q[i] + q[i + 1] if i + 1 < len(q) else q[i] for i in range(0, len(q), 2)]
        return D(v[0]), D(q[0]), np.cumsum(np.asarray(w, D))
    S, Q, c = D(0.0), D(0.0), np.empty(len(w), D)
    for i, x in enumerate(w):
        S = S + D(x)
        Q = Q + D(x) * D(x)
        c[i] = S
    return S, Q, c


def decide(w, any_finite, reward, base, ess_frac, u, defect=None):
    """Rules 3 to 6 for one group, from its weights on: ``(ancestors int32 [n], base' [n], [ESS, S, flag, u])``.  Every operation here is
    one IEEE operation on float64 scalars."""
    n = len(w)
    S, Q, c = serial_sums(w, defect)
    with np.errstate(all="ignore"):
        ess = (S * S) / Q
    u = D(u)
    ident, base = np.arange(n, dtype=np.int32), np.asarray(base, D).copy()
    if not any_finite:
        return ident, base, np.array([ess, S, 2.0, u])
    thr = D(ess_frac) * D(n)
    if not ((ess < thr) if defect == "strict_ess" else (ess <= thr)):
        if defect == "base_on_keep":
            base = np.asarray(reward, D).copy()
        return ident, base, np.array([ess, S, 0.0, u])
    step = S / D(n)
    anc = np.empty(n, np.int32)
    for j in range(n):
        p = (D(j) + u) * step
        hit = np.nonzero(c > p)[0]
        anc[j] = hit[0] if hit.size else n - 1
    return anc, np.asarray(reward, D)[anc].copy(), np.array([ess, S, 1.0, u])


def resample(reward, base, n, lam, ess_frac, seed=0, group_offset=0, event=0, weights=None, u=None, defect=None):
    """All groups.  ``weights`` / ``u`` (per particle / per group): taken as given in place of rules 1-2 / the Philox word - the GPU test
    feeds the kernel's own, after which every operation is exact.  Returns ``(ancestors, weights, base', stats [groups, 4])``."""
    reward, base = np.asarray(reward, D).reshape(-1, n), np.asarray(base, D).reshape(-1, n)
    groups = reward.shape[0]
    anc, wts, nb, stats = np.empty((groups, n), np.int32), np.empty((groups, n), D), np.empty((groups, n), D), np.empty((groups, 4), D)
    for g in range(groups):
        w, ok = weights_of(reward[g], base[g], lam)
        if weights is not None:
            w = np.asarray(weights, D).reshape(-1, n)[g]
        if u is not None:
            ug = D(np.asarray(u, D).reshape(-1)[g])
        elif defect == "u53":
            ug = D((u_word(seed, group_offset + g, event) * (1 << 21) + (1 << 21) - 1)) * D(2.0 ** -53)
        else:
            ug = u_of(seed, group_offset + g, event)
        anc[g], nb[g], stats[g] = decide(w, ok, reward[g], base[g], ess_frac, ug, defect)
        wts[g] = w
    return anc.reshape(-1), wts.reshape(-1), nb.reshape(-1), stats


def gather(src, anc, n, per=1):
    """``dst[(G*n + j)*per + s] = src[(G*n + clamp(anc[G*n + j], 0, n - 1))*per + s]``"""
    src, anc = np.asarray(src), np.clip(np.asarray(anc, np.int64), 0, n - 1)
    particles = anc.size
    v = src.reshape(particles, per, -1)
    rows = (np.arange(particles) // n) * n + anc
    return v[rows].reshape(src.shape)


def lineage(ancestors, n):
    """The events' ancestors composed: int64 ``[groups, n]``, the start particle every final particle descends from."""
    out = None
    for a in ancestors:
        a = np.asarray(a, np.int64).reshape(-1, n)
        out = a if out is None else np.take_along_axis(out, a, axis=1)
    return out


def x0(x, eps, t, table, t_stride=1):
    """``fl(fl(cx*x) - fl(ce*eps))`` per row in float32: ``x`` ``[rows, >= n]``, ``eps`` ``[rows, n]``, ``t`` int64 read at ``r * t_stride``."""
    x, eps = np.asarray(x, F), np.asarray(eps, F)
    rows, n = eps.shape
    out = np.empty_like(eps)
    with np.errstate(all="ignore"):
        for r in range(rows):
            tv = min(max(int(t[r * t_stride]), 0), table.shape[0] - 1)
            cx, ce = F(table[tv, 0]), F(table[tv, 1])
            out[r] = (cx * x[r, :n]).astype(F) - (ce * eps[r]).astype(F)
    return out


def copy_counts_ok(anc, w, n):
    """Systematic resampling: particle i has floor or ceil of ``n * w_i / S`` copies (to within the rounding of that quotient)."""
    w = np.asarray(w, D)
    want = n * w / w.sum()
    cnt = np.bincount(np.asarray(anc), minlength=n)
    return bool(np.all((cnt >= np.floor(want * (1 - 1e-12))) & (cnt <= np.ceil(want * (1 + 1e-12)))))


def steered_at(i, t_value, last, every, window):
    return (i + 1) % every == 0 and window[0] <= t_value <= window[1] and not last


def hand_loop(sampler, steps_mod, x, cond, t_start, steering, reward_fn, *, uncond_scale, uncond_cond, cond_concat=None, event0=0):
    """The steered ``paint`` written by hand: the sampler's own ``get_eps`` and single-step update, numpy in between.  ``sampler`` is built
    WITHOUT steering; ``steps_mod`` is ``polyffusion_amd._steps``.  Returns ``(x, ancestors per event, flags per event)``."""
    import torch
    from polyffusion_amd.sampler import DDIMSampler
    st, n, per = steering, steering.n, steering.per
    ddim = isinstance(sampler, DDIMSampler)
    table = sampler.model.x0_threshold_table(x.device).cpu().numpy()
    window = steering.window_values(sampler.model.n_steps)
    time_steps = np.flip(sampler.time_steps[: t_start + 1])
    rows = x.shape[0]
    base = np.zeros(rows // per)
    wp = sampler.windows
    prep = sampler.prepare(cond, uncond_scale=uncond_scale, uncond_cond=uncond_cond)
    ancs, flags, event = [], [], event0
    for i, step in enumerate(time_steps):
        step, index = int(step), len(time_steps) - i - 1
        t = sampler._t_of(step, sampler._eps_rows(x), x.device)
        xin = x if cond_concat is None else torch.cat([x, cond_concat], dim=1)
        e_t = sampler.get_eps(xin, t, cond, uncond_scale=uncond_scale, uncond_cond=uncond_cond, prep=prep, t_value=step)
        if steered_at(i, step, index == 0, st.every, window):
            xs, es = x.cpu().numpy(), e_t.cpu().numpy()
            p0 = x0(xs.reshape(rows, -1), es.reshape(rows, -1), t.cpu().numpy(), table, 1 if wp is None else wp.n_windows).reshape(es.shape)
            r = reward_fn(torch.from_numpy(p0).to(x.device)).double().cpu().numpy()
            anc, _, base, stats = resample(r, base, n, st.lam, st.ess, sampler.seed, sampler.sample_offset // (n * per), event)
            event += 1
            ancs.append(anc)
            flags.append(stats[:, 2].copy())
            x, e_t = (torch.from_numpy(gather(v, anc, n, per)).to(x.device) for v in (xs, es))
        if ddim:
            x, _ = sampler.get_x_prev_and_pred_x0(e_t, index, x)
        else:
            x = sampler._update(x.contiguous(), e_t, step)[0]
    return x, ancs, flags
