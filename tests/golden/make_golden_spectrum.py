#!/usr/bin/env python
"""Golden vectors of the energy-resolved composition: what flux_averaged_BSMu (golemflavor/fr.py:441-457) computes
per energy bin before it averages.  Run where the reference is available; writes tests/golden/golden_spectrum.npz.

Per configuration (dim, texture), source (1, 2, 0), binning 6e4 1e7 20, 12 theta rows in mc_texture's 7-column layout with logLam
spread over SCALE_BOUNDARIES[dim] (its top included, where the reference's unitarity assert fires), and per (row, bin):
  fr_ref      the reference's u_to_fr(source, params_to_BSMu(..., energy = E_k)) (with check_uni off where it raised)
  ok          0 where params_to_BSMu raised its AssertionError
  abs2_ref    the reference's |U|^2
  abs2_diff   abs2_ref - the exact |U|^2, as float32: on the pairs that pass the assert the difference is below 1e-7 and a float32
              keeps 7 digits of it, so the exact matrix is abs2_ref - abs2_diff to 1e-14 there (where the reference raised its own
              matrix is off by more, and only the size of the difference is of interest)
  fr_exact    the 60-digit composition (tests/exact_mp.py: mp_bsmu + mp_u_to_fr)
and per row the reference's own flux_averaged_BSMu (NaN and status 2 where it raised)."""
import argparse
import collections
import collections.abc
import fractions
import math
import os
import sys

fractions.gcd = math.gcd
collections.Sequence = collections.abc.Sequence
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")

import numpy as np  # noqa: E402

from golemflavor import fr  # noqa: E402
from golemflavor.enums import Likelihood, ParamTag, Texture  # noqa: E402
from golemflavor.param import Param, ParamSet  # noqa: E402

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from exact_mp import mp_abs2, mp_angles_to_u, mp_bsmu, mp_u_to_fr  # noqa: E402

Z = 0. + 1e-9
TEX = {Texture.OEU: (0.5, 1.0, Z, Z), Texture.OET: (Z, 0.25, Z, Z), Texture.OUT: (Z, 1.0, 0.5, Z)}
_orig_bsmu = fr.params_to_BSMu


def _bsmu_shim(bsm_angles, dim, energy, mass_eigenvalues=fr.MASS_EIGENVALUES, sm_u=fr.NUFIT_U,
               no_bsm=False, texture=Texture.NONE, check_uni=True, epsilon=1e-7):
    # the same shim as make_golden.py: `texture is Texture.X` fails across enum re-imports, so the named textures go in as angles
    if texture in TEX:
        sc = bsm_angles[0] if isinstance(bsm_angles, (list, tuple)) else bsm_angles
        bsm_angles = tuple(TEX[texture]) + (sc,)
        texture = Texture.NONE
    return _orig_bsmu(bsm_angles, dim, energy, mass_eigenvalues=mass_eigenvalues, sm_u=sm_u,
                      no_bsm=no_bsm, texture=texture, check_uni=check_uni, epsilon=epsilon)


fr.params_to_BSMu = _bsmu_shim

CONFIGS = [(3, Texture.OET), (6, Texture.OEU), (6, Texture.OUT), (4, Texture.OET)]
SOURCE = (1, 2, 0)
NROWS = 12


def sm6_nuisance():                        # scripts/mc_texture.py:52-76
    tag = ParamTag.SM_ANGLES
    return [
        Param(name='s_12_2', value=0.307, seed=[0.26, 0.35], ranges=[0., 1.], std=0.013, tex=r's_{12}^2', tag=tag),
        Param(name='c_13_4', value=(1 - (0.02206))**2, seed=[0.950, 0.961], ranges=[0., 1.], std=0.00147, tex=r'c_{13}^4', tag=tag),
        Param(name='s_23_2', value=0.538, seed=[0.31, 0.75], ranges=[0., 1.], std=0.069, tex=r's_{23}^2', tag=tag),
        Param(name='dcp', value=4.08404, seed=[0 + 0.1, 2 * np.pi - 0.1], ranges=[0., 2 * np.pi], std=2.0, tex=r'\delta_{CP}', tag=tag),
        Param(name='m21_2', value=7.40E-23, seed=[7.2E-23, 7.6E-23], ranges=[6.80E-23, 8.02E-23], std=2.1E-24, tex=r'\Delta m_{21}^2', tag=tag),
        Param(name='m3x_2', value=2.494E-21, seed=[2.46E-21, 2.53E-21], ranges=[2.399E-21, 2.593E-21], std=3.3E-23, tex=r'\Delta m_{3x}^2', tag=tag),
    ]


def texture_paramset(dimension):
    b = fr.SCALE_BOUNDARIES[dimension]
    return ParamSet(sm6_nuisance() + [Param(name='logLam', value=np.mean(b), ranges=b, std=3, tag=ParamTag.SCALE)])


def main():
    rng = np.random.default_rng(20261018)
    binning = np.logspace(np.log10(6e4), np.log10(1e7), 21)          # scripts/fr.py:122-124
    centres = np.sqrt(binning[:-1] * binning[1:])
    src = fr.normalize_fr(SOURCE)
    out = {k: [] for k in ("theta", "fr_ref", "ok", "abs2_ref", "abs2_diff", "fr_exact", "flux_avg", "flux_status")}
    for dim, tex in CONFIGS:
        ps = texture_paramset(dim)
        lo, hi = fr.SCALE_BOUNDARIES[dim]
        box = np.array(ps.seeds, dtype=float)
        th = rng.uniform(box[:, 0], box[:, 1], size=(NROWS, 7))
        th[:, 6] = np.linspace(lo, hi, NROWS)
        th[0, :6] = [0.307, 0.9564, 0.538, 4.08404, 7.4e-23, 2.494e-21]
        args = argparse.Namespace(binning=binning, source_ratio=src, dimension=dim, no_bsm=False, texture=tex, likelihood=Likelihood.GOLEMFIT)
        c = {k: [] for k in out}
        for row in th:
            sm_u = fr.angles_to_u(list(row[:4]))
            mass = [row[4], row[5]]
            mp_sm = mp_angles_to_u(row[:4])
            r = {k: [] for k in ("fr_ref", "ok", "abs2_ref", "abs2_diff", "fr_exact")}
            for e in centres:
                kw = dict(bsm_angles=[row[6]], dim=dim, energy=e, mass_eigenvalues=mass, sm_u=sm_u, no_bsm=False, texture=tex)
                try:
                    u = fr.params_to_BSMu(**kw)
                    ok = 1
                except AssertionError:
                    u = fr.params_to_BSMu(check_uni=False, **kw)
                    ok = 0
                mu = mp_bsmu(TEX[tex], row[6], dim, e, mass, mp_sm)
                a2 = np.asarray(np.abs(np.asarray(u)) ** 2, dtype=np.float64)
                r["fr_ref"].append(np.asarray(fr.u_to_fr(src, u), dtype=np.float64))
                r["ok"].append(ok)
                r["abs2_ref"].append(a2)
                r["abs2_diff"].append(a2 - mp_abs2(mu))
                r["fr_exact"].append([float(v) for v in mp_u_to_fr(src, mu)])
            for k, v in r.items():
                c[k].append(v)
            try:
                c["flux_avg"].append(np.asarray(fr.flux_averaged_BSMu(list(row), args, -2.0, ps), dtype=np.float64))
                c["flux_status"].append(0)
            except AssertionError:
                c["flux_avg"].append(np.full(3, np.nan))
                c["flux_status"].append(2)
        c["theta"] = th
        for k in out:
            out[k].append(np.asarray(c[k]))
    arrays = {k: np.asarray(v) for k, v in out.items()}
    print("largest |abs2_ref - exact|: %.3e on passing pairs, %.3e on all" % (np.abs(arrays["abs2_diff"][np.asarray(arrays["ok"]) == 1]).max(),
                                                                            np.abs(arrays["abs2_diff"]).max()))
    assert np.abs(arrays["abs2_diff"][np.asarray(arrays["ok"]) == 1]).max() < 1e-7
    arrays["abs2_diff"] = arrays["abs2_diff"].astype(np.float32)
    arrays["ok"] = arrays["ok"].astype(np.int32)
    arrays["flux_status"] = arrays["flux_status"].astype(np.int32)
    arrays["configs"] = np.array([[d, t.value] for d, t in CONFIGS], dtype=np.int32)
    arrays["source"] = np.asarray(src, dtype=np.float64)
    arrays["binning"] = binning
    nraise, npass = int((arrays["ok"] == 0).sum()), int((arrays["ok"] == 1).sum())
    print("pairs: %d raise, %d pass; rows whose flux average raised: %d" % (nraise, npass, int((arrays["flux_status"] == 2).sum())))
    assert nraise >= 20 and npass >= 400
    # a row raises in flux_averaged_BSMu exactly when one of its bins does
    assert np.array_equal(arrays["flux_status"] == 2, (arrays["ok"] == 0).any(axis=2))
    path = os.path.join(HERE, "golden_spectrum.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
