"""A chain in element space on the device: the table the reference's `plot.chainer_plot` builds for `--plot-elements`
(golemflavor/plot.py:528-567) before it draws the triangle -- the four mixing columns replaced by the nine moduli |U_ij|
(`flat_angles_to_u`, fr.py:165-167: abs(angles_to_u(x)) cast to float32), the two source angles by the composition
(`angles_to_fr`, fr.py:82-113), nuisance and scale columns kept.  The kernel is csrc/gf_elements.hip, its arithmetic
csrc/gf_elements.hpp.

What is the reference's and what is this package's own.  The arithmetic, the float32 cast of the moduli and the column ORDER
(nuisance, moduli, scale, fractions; ranges (0, 1) for moduli and fractions) are the reference's (plot.py:538-565).  The reference's
branch cannot run as committed (it reads args.fix_mixing, fix_scale, fix_source_ratio and fix_mixing_almost, which no script
defines, and picks the mixing columns by ParamTag.MMANGLES, which the current scripts' paramsets do not use), so WHICH columns form
the groups is this package's rule (`element_plan`), and so are the output names and the copying of every column the reference's
order does not mention.
"""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import GF_ELEMENT_COPY, GF_ELEMENT_FR3, GF_ELEMENT_MAX_WIDTH, GF_ELEMENT_U9, GfElementGroup, GfElementPlan, check  # noqa: F401
from .enums import ParamTag

U_NAMES = tuple("U_%s%d" % (a, i) for a in ("e", "mu", "tau") for i in (1, 2, 3))
FR_NAMES = ("phi_e", "phi_mu", "phi_tau")


def make_plan(groups, round32=True):
    """A `GfElementPlan` from [(kind, columns)] in output order."""
    if not 1 <= len(groups) <= GF_ELEMENT_MAX_WIDTH:
        raise ValueError("a plan has 1 to %d groups" % GF_ELEMENT_MAX_WIDTH)
    plan = GfElementPlan()
    plan.ngroups, plan.round32 = len(groups), int(bool(round32))
    need = {GF_ELEMENT_COPY: 1, GF_ELEMENT_U9: 4, GF_ELEMENT_FR3: 2}
    for g, (kind, cols) in enumerate(groups):
        cols = [int(c) for c in np.atleast_1d(cols)]
        if kind not in need or len(cols) != need[kind]:
            raise ValueError("group %d: kind %r takes %s columns" % (g, kind, need.get(kind, "no")))
        plan.group[g].kind = kind
        for k, c in enumerate(cols):
            plan.group[g].col[k] = c
    return plan


def plan_width(plan, width_in):
    """The plan's output width for rows of `width_in` columns (gf_element_plan_width); ValueError where the plan is invalid."""
    w = _lib.lib().gf_element_plan_width(C.byref(plan), int(width_in))
    if w < 0:
        raise ValueError("invalid element plan for rows of %d columns" % width_in)
    return int(w)


def element_groups(llh_paramset):
    """(mixing columns or None, source columns or None) by this package's rule: the mixing group is the four MMANGLES parameters if
    the set has exactly four of them, else the first four SM_ANGLES in declaration order (the notebook's convention), else none;
    the source group is the two SRCANGLES parameters if there are exactly two."""
    mm = llh_paramset.from_tag(ParamTag.MMANGLES, index=True)
    sm = llh_paramset.from_tag(ParamTag.SM_ANGLES, index=True)
    src = llh_paramset.from_tag(ParamTag.SRCANGLES, index=True)
    mixing = tuple(mm) if len(mm) == 4 else (tuple(sm[:4]) if len(sm) >= 4 else None)
    return mixing, (tuple(src) if len(src) == 2 else None)


def element_plan(llh_paramset, round32=True):
    """(plan, names, ranges) of the element-space row of a chain sampled over `llh_paramset`.

    Output order (plot.py:544-565): NUISANCE columns, the nine moduli, SCALE columns, the three fractions; then every column not
    consumed by a group and not yet placed, copied in declaration order (this package's addition: nothing sampled disappears).
    ranges: the parameter's own for copied columns, (0, 1) for moduli and fractions.  names: the parameter's for copied columns,
    U_e1 ... U_tau3 and phi_e, phi_mu, phi_tau.  round32: the moduli as float32 values, as the reference's table holds them.
    A set with neither group raises ValueError."""
    mixing, src = element_groups(llh_paramset)
    if mixing is None and src is None:
        raise ValueError("the paramset has neither four mixing columns (MMANGLES or SM_ANGLES) nor two SRCANGLES columns")
    params = list(llh_paramset)
    groups, names, ranges, placed = [], [], [], set(mixing or ()) | set(src or ())

    def copy(c):
        groups.append((GF_ELEMENT_COPY, [c]))
        names.append(params[c].name)
        ranges.append(tuple(float(v) for v in params[c].ranges))
        placed.add(c)

    for c in llh_paramset.from_tag(ParamTag.NUISANCE, index=True):
        if c not in placed:
            copy(c)
    if mixing is not None:
        groups.append((GF_ELEMENT_U9, list(mixing)))
        names += U_NAMES
        ranges += [(0., 1.)] * 9
    for c in llh_paramset.from_tag(ParamTag.SCALE, index=True):
        if c not in placed:
            copy(c)
    if src is not None:
        groups.append((GF_ELEMENT_FR3, list(src)))
        names += FR_NAMES
        ranges += [(0., 1.)] * 3
    for c in range(len(params)):
        if c not in placed:
            copy(c)
    if len(names) > GF_ELEMENT_MAX_WIDTH:
        raise ValueError("the element-space row has %d columns, at most %d are supported" % (len(names), GF_ELEMENT_MAX_WIDTH))
    return make_plan(groups, round32), names, ranges


def element_rows(rows, plan, *, model):
    """Host rows (n, width_in) -- or (nchains, n, width_in) -- in element space: (..., n, width_out), computed on `model`'s
    device (any `Model`, or an object with a `.model`)."""
    x = np.ascontiguousarray(rows, dtype=np.float64)
    if x.ndim not in (2, 3) or x.shape[-1] < 1:
        raise ValueError("rows must be (n, width_in) or (nchains, n, width_in)")
    w = plan_width(plan, x.shape[-1])
    model = getattr(model, "model", model)
    flat = x.reshape(-1, x.shape[-1])
    out = np.empty((flat.shape[0], w))
    check(model._L.gf_element_rows(model._h, flat.ctypes.data_as(_lib._dp), flat.shape[0], flat.shape[1], C.byref(plan),
                                   out.ctypes.data_as(_lib._dp)), "gf_element_rows")
    return out.reshape(x.shape[:-1] + (w,))


def element_rows_device(d_in, nrows, width_in, plan, d_out, *, model):
    """Device rows: d_in [nrows][width_in] -> d_out [nrows][width_out] (device pointers or `Model.alloc` buffers)."""
    model = getattr(model, "model", model)
    check(model._L.gf_element_rows_device(model._h, getattr(d_in, "ptr", d_in), int(nrows), int(width_in), C.byref(plan),
                                          getattr(d_out, "ptr", d_out)), "gf_element_rows_device")
