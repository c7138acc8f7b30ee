"""The reference for DAS gauge channels (parameter key "das_gauge_length", csrc/das_gauge.hpp), shared by every test that compares
them with the CPU oracle.

The oracle knows one-cell channels only.  A gauge channel c at p with G cells along the axis a is  sum_j w_j e(p + k_j a)  over its
members j, so the oracle is given the EXPANDED member survey -- one channel per member, channel-major, same sensitivities -- and

  forward:   gauge_c = sum_j w_j ett_(c, j), formed in float64 from the oracle's member gathers;
  backward:  the gauge misfit 1/2 sum r_c^2 (or the conditioned one) has d / d ett_(c, j) = w_j a_c with a_c the adjoint source of
             channel c, so member j of channel c is handed  w_j a_c  through oracle.cufd(adj_src=...) -- the chain rule of a linear
             map, exact.  tests/test_gauge_reference.py checks that gradient against finite differences of the gauge misfit.

The data-conditioning chain (windows, band-pass, cross-correlation misfit, source update) acts on what the channel records -- the
gauge gathers -- not on its members."""
import numpy as np

from fuzz_common import groups

COND_KEYS = ("if_win", "filter", "if_cross_misfit", "if_src_update")


def members(G):
    """Members k and weights w_k of a gauge of G cells (midpoint rule for odd G, trapezoid rule for even G)."""
    if G % 2:
        ks = np.arange(-(G - 1) // 2, (G - 1) // 2 + 1)
        return ks, np.full(ks.size, 1.0 / G)
    ks = np.arange(-G // 2, G // 2 + 1)
    w = np.full(ks.size, 1.0 / G)
    w[0] = w[-1] = 0.5 / G
    return ks, w


def is_shot(key):
    return key.startswith("shot") and key[4:].isdigit()


def member_survey(survey, G, vertical):
    """Every channel c replaced by its members, channel-major (member j of channel c is channel c * M + j).  The gauge runs along z
    when `vertical` (para "das_fiber": "vertical") and along x otherwise, for straight and for directional channels
    ("das_sensitivity": every member carries its channel's sensitivities); shots may have different channel counts."""
    ks, _ = members(G)
    out = {}
    for key, sh in survey.items():
        if not is_shot(key):
            out[key] = sh
            continue
        z, x = np.asarray(sh["z_rec"], int).reshape(-1), np.asarray(sh["x_rec"], int).reshape(-1)
        zm = (z[:, None] + (ks[None, :] if vertical else 0)) * np.ones((1, ks.size), int)
        xm = (x[:, None] + (0 if vertical else ks[None, :])) * np.ones((1, ks.size), int)
        new = dict(sh, z_rec=zm.ravel().tolist(), x_rec=xm.ravel().tolist(), nrec=int(zm.size))
        if "das_sensitivity" in sh:
            new["das_sensitivity"] = np.repeat(np.asarray(sh["das_sensitivity"], float).reshape(z.size, -1), ks.size, axis=0).tolist()
        out[key] = new
    return out


def gauge_of(member_ett, G):
    """(group, nrec * M, nSteps) member gathers -> (group, nrec, nSteps) gauge gathers, in float64."""
    _, w = members(G)
    g, n, nt = member_ett.shape
    return np.einsum("gcjt,j->gct", member_ett.reshape(g, n // w.size, w.size, nt).astype(np.float64), w)


def centre_of(member_gather, G):
    """(group, nrec * M, nSteps) -> the centre member's gather (group, nrec, nSteps): pr / vx / vz are sampled at the channel's own cell."""
    ks, _ = members(G)
    g, n, nt = member_gather.shape
    return member_gather.reshape(g, n // ks.size, ks.size, nt)[:, :, int(np.where(ks == 0)[0][0])]


def forward(oracle, models, stf, ids, para, survey, G):
    """Member-survey forward pass.  -> per shot of ids (lists, channel counts may differ):  gauge gathers (nrec, nSteps) float64 and
    the (3, nrec, nSteps) float32 pr / vx / vz gathers of the channels' own cells."""
    vertical = para.get("das_fiber", "horizontal") == "vertical"
    plain = {k: v for k, v in para.items() if k not in COND_KEYS + ("das_gauge_length",)}
    msurvey = member_survey(survey, G, vertical)
    lam, mu, den = [np.asarray(m) for m in models]
    gauge, own = [], []
    for grp in groups(ids, survey):
        syn = oracle.cufd(lam, mu, den, np.asarray(stf), 2, np.asarray(grp, np.int32), plain, msurvey)["syn"]
        gg = gauge_of(syn[:, 3], G)
        cc = np.stack([centre_of(syn[:, k], G) for k in range(3)], axis=1)
        for i in range(len(grp)):
            gauge.append(gg[i])
            own.append(cc[i])
    return gauge, own


def reference(oracle, models, stf, ids, para, survey, G, obs_gauge, cond=None):
    """Misfit and gradients of the gauge problem through the oracle.

    models: (Lambda, Mu, Den) as oracle.cufd takes them; para / survey: the problem's dicts WITH the gauge channels (survey) -- the key
    das_gauge_length and the conditioning keys of para are taken out before the oracle sees it; obs_gauge: per shot of ids the observed
    gauge gathers (nrec, nSteps), an array when the shots share nrec.  cond: None -- the conditioning request of para / survey's keys,
    if any (oracle.conditioning_of) --, or a request dict for all shots, or a list of them per shot.  The residual and the plain misfit
    are formed in float64; with conditioning oracle.conditioned_residual runs on the GAUGE gathers.  Shots with different channel
    counts are run one at a time and summed in shot order.

    -> dict(misfit, gLambda, gMu, gDen, gStf (group, nSteps), gauge (list per shot, float64), own (list per shot: pr, vx, vz))."""
    stf = np.asarray(stf)
    all_ids = [int(i) for i in np.asarray(ids).reshape(-1)]
    if cond is None:
        conds = [oracle.conditioning_of(para, survey, i) for i in all_ids]
    elif isinstance(cond, dict):
        conds = [cond] * len(all_ids)
    else:
        conds = list(cond)
    gauge, own = forward(oracle, models, stf, ids, para, survey, G)
    total = 0.0
    adj = []
    for i in range(len(all_ids)):
        o = np.asarray(obs_gauge[i])
        assert o.shape == gauge[i].shape, (o.shape, gauge[i].shape)
        if conds[i] is None:
            a = o.astype(np.float64) - gauge[i]
            a[:, 0] = 0.0                                             # first time sample (gpuMinus)
            total += float(np.sum(a * a))
        else:
            obj, a, _, _ = oracle.conditioned_residual(o.astype(np.float32), gauge[i].astype(np.float32), np.float32(para["dt"]), conds[i])
            total += obj
            a = a.astype(np.float64)
        adj.append(a)
    out = inject(oracle, models, stf, ids, para, survey, G, adj)
    out.update(misfit=0.5 * total, gauge=gauge, own=own)
    return out


def inject(oracle, models, stf, ids, para, survey, G, adj):
    """The oracle's backward pass of the gauge problem with a caller's CHANNEL-space adjoint source: adj per shot of ids (nrec, nSteps),
    a_c = -d misfit / d gauge_c.  Member j of channel c is handed  w_j a_c  (formed in float64, float32 as the oracle takes it) through
    oracle.cufd(adj_src=...) on the member survey, one call per group of fuzz_common.groups, summed in shot order.  models, para, survey
    as `reference` takes them.  -> dict(gLambda, gMu, gDen, gStf (group, nSteps))."""
    vertical = para.get("das_fiber", "horizontal") == "vertical"
    plain = {k: v for k, v in para.items() if k not in COND_KEYS + ("das_gauge_length",)}
    msurvey = member_survey(survey, G, vertical)
    _, w = members(G)
    lam, mu, den = [np.asarray(m) for m in models]
    stf = np.asarray(stf)
    spread = []
    for a in adj:
        a = np.asarray(a, np.float64)
        spread.append((w[None, :, None] * a[:, None, :]).reshape(a.shape[0] * w.size, a.shape[1]).astype(np.float32))
    out = None
    pos = 0
    for grp in groups(ids, survey):
        r = oracle.cufd(lam, mu, den, stf, 1, np.asarray(grp, np.int32), plain, msurvey, adj_src=np.stack(spread[pos:pos + len(grp)]))
        pos += len(grp)
        if out is None:
            out = {k: r[k].copy() for k in ("gLambda", "gMu", "gDen", "gStf")}
        else:
            for k in ("gLambda", "gMu", "gDen"):
                out[k] += r[k]
            out["gStf"] = np.concatenate([out["gStf"], r["gStf"]], axis=0)
    return out
