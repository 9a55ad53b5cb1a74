"""Float64 restatement of dual classifier-free guidance (``polyffusion_amd.sampler.DualScale``), written from the formula alone.

A ``chord+txt`` condition token is ``cat([chord part (split columns), texture part], -1)``; a dropped part takes the unconditional
condition's columns.  With ``a`` the part the order names first and ``b`` the other::

    eps = eps(-, -) + first * (eps(a, -) - eps(-, -)) + second * (eps(a, b) - eps(a, -))

``model(x, cond) -> eps`` is any callable on float64 arrays; nothing here imports the package under test."""
import numpy as np

ORDERS = ("chd,txt", "txt,chd")


def partial(cond, uncond, split, order):
    """``cond`` ([..., d]) with the part named SECOND in ``order`` replaced by ``uncond``'s columns."""
    cond, uncond = np.asarray(cond, dtype=np.float64), np.broadcast_to(np.asarray(uncond, dtype=np.float64), np.shape(cond))
    assert order in ORDERS and 0 < split < cond.shape[-1]
    out = cond.copy()
    if order == "chd,txt":
        out[..., split:] = uncond[..., split:]
    else:
        out[..., :split] = uncond[..., :split]
    return out


def single(model, x, cond, uncond, scale):
    """The reference's ``get_eps`` (``sampler/__init__.py:63-77``) without its exact-float shortcuts."""
    e_u, e_c = model(x, uncond), model(x, cond)
    return e_u + scale * (e_c - e_u)


def dual(model, x, cond, uncond, first, second, split, order="chd,txt"):
    e0, e1, e2 = model(x, np.broadcast_to(uncond, np.shape(cond))), model(x, partial(cond, uncond, split, order)), model(x, cond)
    return e0 + first * (e1 - e0) + second * (e2 - e1)


def reduce(first, second):
    """Which evaluation the exact-float reductions leave: ``("single", scale, which condition)`` or ``("dual",)``."""
    if first == second:
        return ("single", first, "cond")
    if second == 0.0:
        return ("single", first, "partial")
    return ("dual",)


def combine3_f32(e0, e1, e2, s1, s2):
    """``pf_cfg_combine3`` step by step in numpy float32: five individually rounded operations in the documented order."""
    f = np.float32
    e0, e1, e2, s1, s2 = (np.asarray(v, dtype=f) for v in (e0, e1, e2, s1, s2))
    d1 = (e1 - e0).astype(f)
    p1 = (s1 * d1).astype(f)
    a1 = (e0 + p1).astype(f)
    d2 = (e2 - e1).astype(f)
    p2 = (s2 * d2).astype(f)
    return (a1 + p2).astype(f)


def combine2_f32(e0, e1, s):
    f = np.float32
    e0, e1, s = (np.asarray(v, dtype=f) for v in (e0, e1, s))
    return (e0 + (s * (e1 - e0).astype(f)).astype(f)).astype(f)
