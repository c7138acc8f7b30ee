"""Host-side helpers that produce the INPUTS of the propagator (unchanged semantics of the reference's
fwi_utils.py): JSON writers, Ricker source, replicate padding.  Pure numpy / torch."""
from __future__ import annotations

import json
import os

import numpy as np
import torch
import torch.nn.functional as F


def nPad_for(nz: int, nPml: int, multiple: int = 32) -> int:
    """Rows appended below the bottom PML so that nz + 2 nPml + nPad is a multiple of 32
    (Main-001-FWI-Anomaly-Vp-Vs-Den.py:35; yields 32, not 0, when already a multiple)."""
    return int(multiple - np.mod(nz + 2 * nPml, multiple))


def padding_numpy_array(arr: np.ndarray, npml: int, npad: int) -> np.ndarray:
    """Edge-replicate a (nz, nx) array to (nz + 2 npml + npad, nx + 2 npml)   (fwi_utils.py:11-27)."""
    return np.pad(arr, ((npml, npml + npad), (npml, npml)), mode="edge")


def padding(cp, cs, den, nz_orig, nx_orig, nz, nx, nPml, nPad):
    """Bilinear resize to (nz, nx) (identity when sizes agree) then replicate padding; differentiable
    (fwi_utils.py:31-44)."""
    out = []
    for t in (cp, cs, den):
        t4 = t.view(1, 1, nz_orig, nx_orig)
        t4 = F.interpolate(t4, size=(nz, nx), mode="bilinear", align_corners=False)
        t4 = F.pad(t4, pad=(nPml, nPml, nPml, nPml + nPad), mode="replicate")
        out.append(t4.view(nz + 2 * nPml + nPad, nx + 2 * nPml))
    return tuple(out)


def paraGen(nz, nx, dz, dx, nSteps, dt, f0, nPml, nPad, para_fname, survey_fname, data_dir_name,
            if_win=False, filter_para=None, if_src_update=False, scratch_dir_name="", if_cross_misfit=False,
            das_fiber="horizontal", obs_pack_fname=None, conditioning=None, obs_cache_mb=None, das_gauge_length=None, misfit_weights=None,
            if_envelope_misfit=False, if_w2_misfit=False, w2_beta=None, robust_misfit=None, robust_delta=None, robust_quantile=None,
            fk_slowness=None, fk_mode=None):
    """Write the one-line parameter JSON (schema of fwi_utils.py:46-83; nz, nx are the PADDED sizes).
    das_fiber (extension): "horizontal" = axial strain exx = vx(x) - vx(x-1), the reference's live
    choice; "vertical" = ezz = vz(z) - vz(z-1) (recording_ezz / res_injection_ezz, Src/utilities.cu:620-641, which the
    reference only reaches by editing libCUFD.cu).  The key is written only when it is not the default, so default
    files stay byte-identical to the reference's.
    das_gauge_length (extension) [m]: every channel records the mean axial strain over this gauge along the fibre, a whole multiple
    of the grid spacing along it (csrc/das_gauge.hpp); written only when given.
    misfit_weights (extension): dict with keys among "ett" / "vx" / "vz" -- the weights of the axial-strain, vx and vz residuals in
    misfit and adjoint source (csrc/geophone.hpp; defaults ett 1, vx 0, vz 0).  Only the keys given are written.
    if_envelope_misfit (extension): the misfit compares the squared envelopes of the conditioned gathers instead of the gathers
    (include/sepfwi.h, sepfwi_cufd); refused by the library together with if_cross_misfit, if_src_update or misfit_weights.  Written
    only when set.
    if_w2_misfit / w2_beta (extension): the misfit is the trace-wise quadratic Wasserstein distance between the softplus densities of the
    conditioned gathers, softplus(w2_beta x / max |observed trace|) (include/sepfwi.h, sepfwi_cufd); w2_beta in (0, 16], the library's
    default 3.  Refused by the library together with if_cross_misfit, if_envelope_misfit, if_src_update or misfit_weights.  Each key is
    written only when set.
    robust_misfit / robust_delta / robust_quantile (extension): robust_misfit "huber" or "cauchy" makes the misfit that penalty of the
    conditioned residual, with the threshold robust_delta A per trace, A the order statistic floor(robust_quantile (n - 1)) of the n live
    samples |C obs| (csrc/robust_misfit.hpp).  robust_delta is required with robust_misfit (finite, > 0; no default: it depends on the
    data's noise), robust_quantile in (0, 1], the library's default 0.9; either without robust_misfit is refused, here as in the library.
    Refused by the library together with if_cross_misfit, if_envelope_misfit, if_w2_misfit, if_src_update or misfit_weights.  Each key is
    written only when set.
    fk_slowness / fk_mode (extension): fk_slowness [p1, p2, p3, p4] in s/m switches on the apparent-slowness (f-k) fan filter across every
    shot's channels, the third stage of the conditioning chain (C = FK . band-pass . window; csrc/conditioning.hpp, fk_filter): four finite
    numbers p1 < p2 <= p3 < p4, p > 0 an event that arrives later at higher channel indices; fk_mode "pass" (the library's default) keeps the
    band, "reject" removes it; fk_mode without fk_slowness is refused, here as in the library.  The survey's channels must lie on one
    straight, equally spaced line per shot (the library refuses the session otherwise); refused together with misfit_weights.  Each key is
    written only when set."""
    para = {"nz": int(nz), "nx": int(nx), "dz": dz, "dx": dx, "nSteps": int(nSteps), "dt": float(dt),
            "f0": f0, "nPoints_pml": int(nPml), "nPad": int(nPad)}
    if if_win:
        para["if_win"] = True
    if filter_para is not None:
        para["filter"] = filter_para
    if if_src_update:
        para["if_src_update"] = True
    para["survey_fname"] = survey_fname
    para["data_dir_name"] = data_dir_name
    os.makedirs(data_dir_name, exist_ok=True)
    if if_cross_misfit:
        para["if_cross_misfit"] = True
    if if_envelope_misfit:
        para["if_envelope_misfit"] = True
    if if_w2_misfit:
        para["if_w2_misfit"] = True
    if w2_beta is not None:
        if not (np.isfinite(w2_beta) and 0 < w2_beta <= 16):
            raise ValueError("w2_beta must be in (0, 16]")
        para["w2_beta"] = float(w2_beta)
    if robust_misfit is not None:
        if robust_misfit not in ("huber", "cauchy"):
            raise ValueError("robust_misfit must be 'huber' or 'cauchy'")
        if robust_delta is None:
            raise ValueError("robust_misfit needs robust_delta (finite, > 0; there is no default)")
        para["robust_misfit"] = robust_misfit
    elif robust_delta is not None or robust_quantile is not None:
        raise ValueError("%s without robust_misfit" % ("robust_delta" if robust_delta is not None else "robust_quantile"))
    if robust_delta is not None:
        if not (np.isfinite(robust_delta) and robust_delta > 0):
            raise ValueError("robust_delta must be finite and > 0")
        para["robust_delta"] = float(robust_delta)
    if robust_quantile is not None:
        if not 0 < robust_quantile <= 1:
            raise ValueError("robust_quantile must be in (0, 1]")
        para["robust_quantile"] = float(robust_quantile)
    if fk_slowness is not None:
        p = [float(v) for v in fk_slowness]
        if len(p) != 4 or not all(np.isfinite(v) for v in p) or not (p[0] < p[1] <= p[2] < p[3]):
            raise ValueError("fk_slowness must be four finite numbers p1 < p2 <= p3 < p4")
        para["fk_slowness"] = p
    if fk_mode is not None:
        if fk_mode not in ("pass", "reject"):
            raise ValueError("fk_mode must be 'pass' or 'reject'")
        if fk_slowness is None:
            raise ValueError("fk_mode without fk_slowness")
        para["fk_mode"] = fk_mode
    if das_fiber != "horizontal":
        if das_fiber != "vertical":
            raise ValueError("das_fiber must be 'horizontal' or 'vertical'")
        para["das_fiber"] = das_fiber
    if das_gauge_length is not None:
        if not das_gauge_length > 0:
            raise ValueError("das_gauge_length must be > 0")
        para["das_gauge_length"] = float(das_gauge_length)
    if misfit_weights is not None:
        for k, v in misfit_weights.items():
            if k not in ("ett", "vx", "vz"):
                raise ValueError("misfit_weights keys must be among 'ett', 'vx', 'vz'")
            if not (np.isfinite(v) and v >= 0):
                raise ValueError("misfit_weights values must be finite and >= 0")
            para["misfit_w_" + k] = float(v)
    if scratch_dir_name != "":
        para["scratch_dir_name"] = scratch_dir_name
        os.makedirs(scratch_dir_name, exist_ok=True)
    if conditioning is not None:   # "live" (default behaviour of this library) or "reference": if_win / filter / if_src_update / if_cross_misfit
        if conditioning not in ("live", "reference"):   # are parsed and ignored, as the reference's driver does (libCUFD.cu:353-457)
            raise ValueError("conditioning must be 'live' or 'reference'")
        para["conditioning"] = conditioning
    if obs_cache_mb:        # extension: HBM budget [MB] of the session's observed-data store (beyond it: pinned host memory)
        para["obs_cache_mb"] = int(obs_cache_mb)
    if obs_pack_fname:      # extension: one packed file of axial-strain gathers instead of four files per shot
        para["obs_pack_fname"] = obs_pack_fname
    with open(para_fname, "w") as fp:
        json.dump(para, fp)


def surveyGen(z_src, x_src, z_rec, x_rec, survey_fname, Windows=None, Weights=None, Src_Weights=None, Src_rxz=None, Rec_rxz=None,
              Das_sensitivity=None):
    """Write the one-line survey JSON: every shot shares the receiver list; indices are UNPADDED grid
    indices (fwi_utils.py:87-124).
    Das_sensitivity (extension): (nrec, 6) directional sensitivities of the DAS channels in the layout of
    the reference's Numba solver (DAS_Waveform_Modeling/src/elasticSolver.py:152-153,276): column 0 weighs exx, column 3
    ezz, column 1 exz -- ett = s0 exx + s3 ezz + s1 exz, for shaped / dipping fibres.  Omitted: a straight fibre along x
    (or z, parameter key das_fiber), the reference's CUDA behaviour; the key is only written when given."""
    z_src = np.asarray(z_src).tolist()
    x_src = np.asarray(x_src).tolist()
    z_rec = np.asarray(z_rec).tolist()
    x_rec = np.asarray(x_rec).tolist()
    survey = {"nShots": len(x_src)}
    for i in range(len(x_src)):
        shot = {"z_src": int(z_src[i]), "x_src": int(x_src[i]), "nrec": len(x_rec),
                "z_rec": [int(v) for v in z_rec], "x_rec": [int(v) for v in x_rec]}
        if Windows is not None:
            shot["win_start"] = [float(v) for v in Windows["shot%d" % i]["start"]]
            shot["win_end"] = [float(v) for v in Windows["shot%d" % i]["end"]]
        if Weights is not None:
            shot["weights"] = [float(v) for v in Weights["shot%d" % i]["weights"]]
        if Src_Weights is not None:
            shot["src_weight"] = Src_Weights[i]
        if Src_rxz is not None:
            shot["src_rxz"] = Src_rxz[i]
        if Rec_rxz is not None:
            shot["rec_rxz"] = np.asarray(Rec_rxz).tolist()
        if Das_sensitivity is not None:
            ds = np.asarray(Das_sensitivity, dtype=float)
            if ds.shape != (len(x_rec), 6):
                raise ValueError("Das_sensitivity must be (nrec, 6): exx, exz, -, ezz, -, - (elasticSolver.py:152-153)")
            shot["das_sensitivity"] = ds.tolist()
        survey["shot%d" % i] = shot
    with open(survey_fname, "w") as fp:
        json.dump(survey, fp)


_PARA_KEYS = ("nz", "nx", "nSteps", "nPad", "dx", "dz", "survey_fname")
_FILE_CACHE = {}   # ONE entry per kind of file: "para" / "survey" -> ((path, st_mtime_ns, st_size), what the Python side needs of it)


def _cached_line(kind, fname, digest):
    """digest(the one JSON line of fname), read again only when the file's path, mtime or size has changed"""
    st = os.stat(fname)
    key = (str(fname), st.st_mtime_ns, st.st_size)
    hit = _FILE_CACHE.get(kind)
    if hit is None or hit[0] != key:
        with open(fname) as fp:
            hit = _FILE_CACHE[kind] = (key, digest(json.loads(fp.readline())))
    return hit[1]


def read_para(para_fname):
    """What the Python side reads of a parameter file: those of nz, nx, nSteps, nPad, dx, dz, survey_fname that it holds, as a dict.
    Raises what open / json raise on a missing or malformed file."""
    return _cached_line("para", para_fname, lambda j: {k: j[k] for k in _PARA_KEYS if k in j})


def read_survey_channels(para_fname):
    """{"shot<id>": channel count} of the survey file that the parameter file names."""
    return _cached_line("survey", read_para(para_fname)["survey_fname"],
                        lambda j: {k: len(v["z_rec"]) for k, v in j.items() if isinstance(v, dict) and "z_rec" in v})


def sourceGene(f, nStep, delta_t):
    """Ricker wavelet, delay 1.2/f, amplitude 1e7, float64 (fwi_utils.py:127-140)."""
    e = np.pi * np.pi * f * f
    tau = delta_t * np.arange(nStep) - 1.2 / f
    return (1.0 - 2.0 * e * tau ** 2) * np.exp(-e * tau ** 2) * 1.0e7


def pseudo_hessian_vp_vs_den(hL, hM, hD, Vp, Vs, Den):
    """Diagonal pseudo-Hessian of (Lambda [MPa], Mu [MPa], Den) -> that of (Vp, Vs, Den), all on the padded grid: the squared partials
    of the map Lambda = (Vp^2 - 2 Vs^2) Den / 1e6, Mu = Vs^2 Den / 1e6 (FWI_ops.py:124-125) weight the three inputs,
        hVp  = (2 Den Vp / 1e6)^2 hL
        hVs  = (4 Den Vs / 1e6)^2 hL + (2 Den Vs / 1e6)^2 hM
        hDen = ((Vp^2 - 2 Vs^2) / 1e6)^2 hL + (Vs^2 / 1e6)^2 hM + hD
    i.e. the column sums of squares of the map's Jacobian.  Cell by cell: the sum over the replicated rim that the padding's
    transpose applies to a gradient (padding()) is NOT applied here -- crop the physical grid out of the result.
    -> (hVp, hVs, hDen)."""
    hVp = (2.0 * Den * Vp / 1e6) ** 2 * hL
    hVs = (4.0 * Den * Vs / 1e6) ** 2 * hL + (2.0 * Den * Vs / 1e6) ** 2 * hM
    hDen = ((Vp ** 2 - 2.0 * Vs ** 2) / 1e6) ** 2 * hL + (Vs ** 2 / 1e6) ** 2 * hM + hD
    return hVp, hVs, hDen


def read_shot_gather(data_dir, comp, shot_id, nSteps):
    """Shot_{pr|vx|vz|ett}{id}.bin -> (nrec, nSteps) float32 (libCUFD.cu:755-769)."""
    return np.fromfile(os.path.join(data_dir, "Shot_%s%d.bin" % (comp, shot_id)), dtype=np.float32).reshape(-1, nSteps)


PACK_MAGIC = b"SEPFWIP1"


def pack_observed(data_dir, shot_ids, nSteps, pack_fname):
    """One file for a whole survey's observed axial-strain gathers instead of the reference's four files per
    shot, of which only Shot_ett{id}.bin enters misfit and adjoint source (Src/libCUFD.cu:216-223,427,607).  Layout, little
    endian:  8 bytes magic "SEPFWIP1" | int32 nEntries | int32 nSteps | nEntries x (int32 shot_id, int32 nrec, int64 byte offset)
    | the gathers, float32 [nrec][nSteps] each, exactly the bytes of the Shot_ett files.  Named by the parameter key
    "obs_pack_fname" (paraGen(..., obs_pack_fname=)); shots missing from the pack are still read from their own files."""
    ids = [int(i) for i in shot_ids]
    gathers = [read_shot_gather(data_dir, "ett", i, nSteps) for i in ids]
    head = 8 + 8 + 16 * len(ids)
    off = head
    with open(pack_fname, "wb") as fp:
        fp.write(PACK_MAGIC)
        fp.write(np.array([len(ids), nSteps], dtype="<i4").tobytes())
        for i, g in zip(ids, gathers):
            fp.write(np.array([i, g.shape[0]], dtype="<i4").tobytes())
            fp.write(np.array([off], dtype="<i8").tobytes())
            off += g.size * 4
        for g in gathers:
            fp.write(np.ascontiguousarray(g, dtype="<f4").tobytes())
    return pack_fname


def read_packed_gather(pack_fname, shot_id):
    """-> (nrec, nSteps) float32 of one shot of a pack_observed file."""
    with open(pack_fname, "rb") as fp:
        if fp.read(8) != PACK_MAGIC:
            raise ValueError("%s is not a packed observed-data file" % pack_fname)
        n, nSteps = np.frombuffer(fp.read(8), dtype="<i4")
        for _ in range(int(n)):
            sid, nrec = np.frombuffer(fp.read(8), dtype="<i4")
            off = int(np.frombuffer(fp.read(8), dtype="<i8")[0])
            if int(sid) == int(shot_id):
                fp.seek(off)
                return np.frombuffer(fp.read(int(nrec) * int(nSteps) * 4), dtype="<f4").reshape(int(nrec), int(nSteps)).copy()
    raise KeyError("shot %d is not in %s" % (shot_id, pack_fname))


# Mineral / fluid constants of the reference's rock-physics maps (fwi_utils.py:156-167,311-322; FWI_ops.py:452-462,573-584):
# quartz, clay, water, hydrocarbon; cs = consolidation parameter of the drained frame (Dupuy et al. 2016).
ROCK = dict(k_q=37.00 * 1e9, k_c=21.00 * 1e9, k_w=2.25 * 1e9, k_h=0.04 * 1e9, mu_q=44.00 * 1e9, mu_c=10.00 * 1e9,
            rho_q=2.65 * 1e3, rho_c=2.55 * 1e3, rho_w=1.00 * 1e3, rho_h=0.10 * 1e3, cs=20.0)


def pcs2dv_vrh(phi, cc, sw):
    """(porosity, clay content, water saturation) -> (vp, vs, rho), Voigt-Reuss-Hill   (fwi_utils.py:154-196)."""
    R = ROCK
    kv = (1 - phi) * (R["k_c"] * cc + R["k_q"] * (1 - cc)) + phi * (R["k_w"] * sw + R["k_h"] * (1 - sw))
    kr_1 = (1 - phi) * (cc / R["k_c"] + (1 - cc) / R["k_q"]) + phi * (sw / R["k_w"] + (1 - sw) / R["k_h"])
    k = 0.5 * (kv + 1 / kr_1)
    mu = 0.5 * ((1 - phi) * (R["mu_c"] * cc + R["mu_q"] * (1 - cc)) + 0)
    rho = (R["rho_w"] * sw + R["rho_h"] * (1 - sw)) * phi + (R["rho_c"] * cc + R["rho_q"] * (1 - cc)) * (1 - phi)
    lam = k - 2. / 3. * mu
    return np.sqrt((lam + 2. * mu) / rho), np.sqrt(mu / rho), rho


def pcs2dv_gassmann(phi, cc, sw):
    """(porosity, clay content, water saturation) -> (vp, vs, rho), Biot-Gassmann with Voigt mineral mixing
    (fwi_utils.py:309-352: weighted_average, vrh(method='Voigt'), drained_moduli, biot_gassmann)."""
    R = ROCK
    rho_f = R["rho_w"] * sw + R["rho_h"] * (1 - sw)
    k_f = R["k_w"] * sw + R["k_h"] * (1 - sw)
    k_s = R["k_c"] * cc + R["k_q"] * (1 - cc)
    mu_s = R["mu_c"] * cc + R["mu_q"] * (1 - cc)
    rho_s = R["rho_c"] * cc + R["rho_q"] * (1 - cc)
    k_d = k_s * ((1 - phi) / (1 + R["cs"] * phi))
    mu_d = mu_s * ((1 - phi) / (1 + 1.5 * R["cs"] * phi))
    delta = ((1 - phi) / phi) * (k_f / k_s) * (1 - (k_d / (k_s - k_s * phi)))
    k_u = (phi * k_d + (1 - (1 + phi) * (k_d / k_s)) * k_f) / (phi * (1 + delta))
    rho = rho_f * phi + rho_s * (1 - phi)
    return np.sqrt((k_u + 0.75 * mu_d) / rho), np.sqrt(mu_d / rho), rho
