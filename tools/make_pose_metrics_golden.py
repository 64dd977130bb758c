#!/usr/bin/env python3
"""Writes tests/golden/pose_metrics.npz: inputs and the REFERENCE's own outputs for the pose-error stage and its AUC - numeric arrays
only.  The reference's utils/metrics.py is loaded on its own (importlib, by path) with an empty stand-in module for cv2, which
angle_error_mat, angle_error_vec, error_auc and aggregate_metrics never reach; nothing else of the reference is imported.  The
inputs come from tests/pose_error_cases.py's seeded generators, so the fixture and the tests have one source.

  pose_R, pose_t, pose_R_gt, pose_t_gt     pose_sets(SEED_POSE, N_POSE): rotations from identical (angles down to 1e-7 rad) to pi,
                                           translations parallel, opposite, orthogonal and in between
  pose_err_R, pose_err_t                   angle_error_mat(R, R_gt); angle_error_vec(t, t_gt) folded as metrics.py:63 folds it
  pose_T0, pose_T1                         extrinsic_sets(SEED_T, ...): inputs only - compute_pose_error needs OpenCV; the test
                                           forms T1 inv(T0) with numpy and applies the two functions' recorded behaviour
  auc_<name>_err_R, auc_<name>_err_t       error_lists(SEED_AUC): n = 0, 1, 2, 3, 15, 64, 65, 1000, 4000 plain and with a fifth inf,
                                           and one list with entries exactly 5, 10 and 20
  auc_<name>_ref [3], auc_<name>_below [3] aggregate_metrics(err_R, err_t) (auc@5, @10, @20; error_auc on the maxima gives the same
                                           bits, asserted here) and error_auc's own last_index - 1: the entries strictly below

usage: make_pose_metrics_golden.py [--reference /path/to/reference]"""
import argparse
import importlib.util
import os
import sys
import types

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))
from ref_import import REF_ROOT                       # where the reference tree lies (PATS_REFERENCE_ROOT); nothing of it is loaded by that import
SEED_POSE, N_POSE, SEED_T, SEED_AUC = 9101, 132, 9102, 9103


def load_metrics(root):
    path = os.path.join(root, "utils", "metrics.py")
    if not os.path.isfile(path):
        raise SystemExit("make_pose_metrics_golden: no utils/metrics.py under %s" % root)
    sys.modules.setdefault("cv2", types.ModuleType("cv2"))             # imported at the top of the file, used by compute_pose_error only
    sys.dont_write_bytecode = True
    spec = importlib.util.spec_from_file_location("reference_metrics", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=REF_ROOT)
    args = ap.parse_args()
    import pose_error_cases as pe
    m = load_metrics(args.reference)
    R, t, Rg, tg = pe.pose_sets(SEED_POSE, N_POSE)
    err_R = np.array([m.angle_error_mat(R[i], Rg[i]) for i in range(N_POSE)], np.float64)
    e = np.array([m.angle_error_vec(t[i], tg[i]) for i in range(N_POSE)], np.float64)
    err_t = np.minimum(e, 180 - e)
    T0, T1 = pe.extrinsic_sets(SEED_T, Rg, tg)
    out = {"pose_R": R, "pose_t": t, "pose_R_gt": Rg, "pose_t_gt": tg, "pose_err_R": err_R, "pose_err_t": err_t, "pose_T0": T0,
           "pose_T1": T1}
    for name, (eR, eT) in pe.error_lists(SEED_AUC).items():
        ref = m.aggregate_metrics(list(eR), list(eT))
        errors = np.maximum(eR, eT)
        assert ref == m.error_auc(errors, [5, 10, 20])
        with_zero = [0] + sorted(list(errors))
        out["auc_%s_err_R" % name], out["auc_%s_err_t" % name] = eR, eT
        out["auc_%s_ref" % name] = np.array([ref["auc@5"], ref["auc@10"], ref["auc@20"]], np.float64)
        out["auc_%s_below" % name] = np.array([np.searchsorted(with_zero, thr) - 1 for thr in (5, 10, 20)], np.int64)
    path = os.path.join(REPO, "tests", "golden", "pose_metrics.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
