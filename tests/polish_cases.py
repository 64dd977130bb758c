"""The per-pair local optimisation of include/pats_amd.h ("Per-pair local optimisation") restated in numpy float64, and the seeded
inputs of its tests.  Shared by tests/test_polish_cases_host.py (CPU) and tests/test_polish_gpu.py; written from the header's
definition alone.

Definition (per pair):  m_0 = the input model;  round r = 1 .. T:  m_r = refit_F(M_{r-1}, c_{r-1}),  (c_r, M_r) = support(m_r);
b = the lowest r in 0 .. T with the largest c_r.  The restatement evaluates the test and the moments in float64 and the refit with
numpy's eigh / svd; each m_r is rounded to float32 as the definition says.  The device evaluates the test in float32, so a
handful of borderline matches may fall the other way - the GPU tests therefore compare the device with the chain of the device's own
entry points (exactly), and use this restatement only to CHOOSE inputs: seeds where the effect asked for is far larger than that."""
import numpy as np

import epipolar_cases as ec
import homography_cases as hcs
import pose_cases as pc

MIN_INLIERS = {"epipolar": 8, "homography": 4}
MAX_ROUNDS = 16
THR = np.float32(2e-3)


def support64(family, xl, xr, part, m, thr):
    """(count, moments [9,9], mask [n]) of the one float32 model m, float64 arithmetic."""
    m = np.asarray(m, np.float32).reshape(1, 3, 3)
    inl = (ec.classify if family == "epipolar" else hcs.classify)(xl, xr, part, m, thr)[0][0]
    if family == "epipolar":
        M = ec.moments64(xl, xr, inl)[0] if inl.any() else np.zeros((9, 9))
    else:
        M = hcs.moments64(xl, xr, inl) if inl.any() else np.zeros((9, 9))
    return int(inl.sum()), M, inl


def refit64(family, M, c):
    """refit_F(M, c) -> [3,3] float32; the zero model where the definition has no model."""
    zero = np.zeros((3, 3), np.float32)
    if c < MIN_INLIERS[family] or not np.isfinite(M).all():
        return zero
    e = pc.refit64(M)[0]
    if family == "epipolar":
        U, s, V = pc.svd_pos(e)
        if not s[1] > 0:
            return zero
        return pc.project64(e).astype(np.float32)
    return hcs.sign_rule(e / np.linalg.norm(e)).reshape(3, 3).astype(np.float32)


def walk64(family, xl, xr, m0, thr, rounds, part=None):
    """The definition -> dict(counts [T + 1], best_round, best_count, models [T + 1,3,3] float32, masks)."""
    part = ec.participates(xl, xr) if part is None else part
    models, counts, masks = [np.asarray(m0, np.float32).reshape(3, 3)], [], []
    for r in range(rounds + 1):
        c, M, inl = support64(family, xl, xr, part, models[r], thr)
        counts.append(c)
        masks.append(inl)
        if r < rounds:
            models.append(refit64(family, M, c))
    b = int(np.argmax(counts))                          # the lowest index of the largest count
    return {"counts": np.asarray(counts, np.int32), "best_round": b, "best_count": counts[b], "models": np.stack(models), "masks": masks}


# ---- cases ----------------------------------------------------------------------------------------------------------------------
def minimal_model(family, xl, xr, idx):
    """The float32 model through the sample idx (8 matches: the 8-point null vector; 4: the DLT's), the sign rule applied."""
    if family == "epipolar":
        l = np.concatenate([xl[idx].astype(np.float64), np.ones((len(idx), 1))], 1)
        r = np.concatenate([xr[idx].astype(np.float64), np.ones((len(idx), 1))], 1)
        A = (r[:, :, None] * l[:, None, :]).reshape(len(idx), 9)
        e = np.linalg.svd(A)[2][-1]
    else:
        e = hcs.null64(hcs.rows(xl, xr, np.asarray(idx)[None, :]))[0]
    return hcs.sign_rule(e / np.linalg.norm(e)).reshape(3, 3).astype(np.float32)


def make_pair(family, seed, n, outliers=0.4, noise=None):
    """One planted pair - epipolar_cases.make_case's two-view distributions (pose_cases.make_scene) or homography_cases' plane - and a
    NOISY MINIMAL-SAMPLE model: the model through 8 (4) of its true matches, drawn by the seed, noise and all.
    -> dict(ml, mr, good, model [3,3] float32, thr)."""
    kw = {} if noise is None else {"noise": noise}
    s = (pc.make_scene if family == "epipolar" else hcs.make_scene)(seed, n, outliers=outliers, **kw)
    rng = np.random.default_rng(seed + 104729)
    idx = rng.choice(np.flatnonzero(s["good"]), MIN_INLIERS[family], replace=False)
    return {"ml": s["ml"], "mr": s["mr"], "good": s["good"], "model": minimal_model(family, s["ml"], s["mr"], idx), "thr": THR}


# "it helps": (family, seed, matches) - the float64 walk of 4 rounds gains at least GAIN * n inliers over the minimal-sample model.
# Found by scanning seeds 1 .. 40 per family with the functions above; only such seeds are kept.
GAIN = 0.05
HELPS_ROUNDS = 4
HELPS = [("epipolar", 1, 600), ("epipolar", 4, 600), ("epipolar", 13, 600), ("epipolar", 24, 600),
         ("homography", 2, 600), ("homography", 4, 600), ("homography", 12, 600), ("homography", 37, 600)]

# "keeps the best": (family, seed, matches, outliers, noise, rounds) - the float64 walk reaches its largest count before the last round
# and ends at least KEEPS_MARGIN inliers below it (a margin no float32 borderline verdict bridges).  Found by scanning seeds 1 .. 59
# of both families; the homography walks found were all monotone, so the cases are epipolar.
KEEPS_MARGIN = 8
KEEPS = [("epipolar", 26, 600, 0.4, None, 4), ("epipolar", 40, 600, 0.4, None, 4), ("epipolar", 15, 400, 0.5, 1e-3, 3),
         ("epipolar", 27, 400, 0.7, 1e-3, 3)]


def helps_cases():
    return [(f, make_pair(f, seed, n)) for f, seed, n in HELPS]


def keeps_cases():
    return [(f, rounds, make_pair(f, seed, n, outliers=out, noise=noise)) for f, seed, n, out, noise, rounds in KEEPS]


# ---- the C entry points' refusals -------------------------------------------------------------------------------------------------
# the argument order of the two prototypes (before workspace, workspace_bytes, stream), the pointers that must not be null, every
# pointer's alignment, the scalars of a valid call
ENTRY = {"epipolar": ("pats_epipolar_polish_by_pair_f32", b"epipolar_polish_by_pair"),
         "homography": ("pats_homography_polish_by_pair_f32", b"homography_polish_by_pair")}
ORDER = ("matches_l", "matches_r", "conf", "pair_off", "stride", "counts_in", "pairs", "cap", "thr", "norm", "use_min_conf", "min_conf",
         "models", "H", "best", "rounds", "model", "best_count", "inlier", "moments", "best_round", "counts")
REQUIRED = ("matches_l", "matches_r", "models", "thr", "model", "best_count", "inlier", "moments", "best_round", "counts")
ALIGN = {"matches_l": 8, "matches_r": 8, "models": 4, "thr": 4, "model": 4, "best_count": 8, "moments": 8, "best_round": 4, "counts": 4,
         "conf": 4, "norm": 4, "pair_off": 8, "counts_in": 8, "best": 4, "inlier": 1}
SCALARS = {"stride": 0, "pairs": 2, "cap": 100, "use_min_conf": 0, "min_conf": 0.0, "H": 8, "rounds": 4}


def c_call(lib, family, base, ws_bytes=1 << 20, **kw):
    """One raw call of an entry point with `base` behind every pointer (the ragged form), `kw` overriding arguments by name."""
    import ctypes
    a = {n: base for n in ALIGN}
    a["counts_in"] = 0
    a.update(SCALARS)
    a.update(kw)
    args = [(ctypes.c_void_p(a[n]) if a[n] else None) if n in ALIGN else a[n] for n in ORDER]
    return getattr(lib, ENTRY[family][0])(*args, ctypes.c_void_p(base), ws_bytes, None)


def refusals(lib, base):
    """Every refusal of the header's list -> [(keyword arguments of c_call(), the words the message must hold)]."""
    max_h = lib.pats_epipolar_max_h()
    strided = {"pair_off": 0, "counts_in": base}
    out = [({name: 0}, (b"null", name.encode())) for name in REQUIRED]
    for name, al in sorted(ALIGN.items()):
        if al == 1:
            continue
        form = dict(strided, stride=10) if name == "counts_in" else {}
        out += [(dict(form, **{name: base + off}), (b"%d-byte aligned" % al, name.encode())) for off in ((1, 2, 3) if al == 4 else (1, 2, 4))]
    out += [(kw, (word,)) for kw, word in (({"pairs": 0}, b"pairs"), ({"pairs": -3}, b"pairs"), ({"H": 0}, b"H ="), ({"H": -1}, b"H ="),
                                           ({"H": max_h + 1}, b"max_h"))]
    out += [(dict(strided, pair_off=base, stride=10), (b"pair_off", b"counts_in")), ({"pair_off": 0}, (b"pair_off", b"counts_in"))]
    out += [(kw, (b"cap",)) for kw in ({"cap": -1}, {"cap": 2 ** 31 - 1}, {"cap": 2 ** 40})]
    out += [(dict(strided, **kw), (b"stride",)) for kw in ({"stride": 0}, {"stride": -4}, {"stride": 51}, {"stride": 10, "pairs": 11},
                                                            {"stride": 1, "cap": 0})]
    out += [({"use_min_conf": 1, "min_conf": bad}, (b"min_conf",)) for bad in (float("nan"), -0.25, float("-inf"))]
    out += [({"use_min_conf": 1, "min_conf": 0.5, "conf": 0}, (b"min_conf", b"conf"))]
    out += [({"rounds": bad}, (b"rounds",)) for bad in (0, -1, MAX_ROUNDS + 1, 2 ** 20)]
    out += [({"best": 0, "H": 2}, (b"best", b"H")), ({"best": 0, "H": max_h}, (b"best", b"H"))]
    return out


def check_refusals(lib, family, base):
    """Every refusal is refused with a message that names the entry point and the argument -> the number of cases."""
    cases = refusals(lib, base)
    for kw, words in cases:
        assert c_call(lib, family, base, **kw) != 0, (family, kw)
        msg = lib.pats_last_error()
        assert ENTRY[family][1] in msg and all(w in msg for w in words), (family, kw, msg)
    return len(cases)
