#!/usr/bin/env python3
"""Writes tests/golden/prepare_intrinsics.npz: the REFERENCE's own outputs for the intrinsics of the image front end - numbers only,
a few KB.  The reference's Get_resize_ratio, Create_K_resize (the three lines datasets/yfcc.py:39-42 apply, as a function) and
scale_intrinsics are imported through tools/ref_import.py (numpy-only; cv2 is stubbed there) and called on the size combinations
and seeded intrinsics of tests/prepare_cases.py, so the fixture and the tests have one source.

  sizes [n,4] int64       (w0, h0, w_t, h_t) per combination
  K [n,3,3]               the raw image's intrinsics (prepare_cases.intrinsic_K)
  ratio [n], add_num [n,2]  Get_resize_ratio(np.array([w0, h0]), np.array([w_t, h_t]))
  K_ratio [n,3,3]         Create_K_resize(K, K, (w0, h0), (w0, h0), shape=(w_t, h_t))[0][:3, :3]
  K_axes [n,3,3]          scale_intrinsics(K, [float(w0) / w_t, float(h0) / h_t])   (datasets/scannet.py:54)

usage: make_golden_prepare.py"""
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tests"))
sys.path.insert(0, os.path.join(REPO, "tools"))


def main():
    import prepare_cases as pc
    import ref_import
    U = ref_import.load().U
    n = len(pc.INTRINSIC_SIZES)
    out = {"sizes": np.zeros((n, 4), np.int64), "K": np.zeros((n, 3, 3)), "ratio": np.zeros(n), "add_num": np.zeros((n, 2)),
           "K_ratio": np.zeros((n, 3, 3)), "K_axes": np.zeros((n, 3, 3))}
    for i, ((w0, h0), (w_t, h_t)) in enumerate(pc.INTRINSIC_SIZES):
        K = pc.intrinsic_K(i)
        origin, shape = np.array([w0, h0]), np.array([w_t, h_t])
        out["sizes"][i], out["K"][i] = (w0, h0, w_t, h_t), K
        out["ratio"][i], out["add_num"][i] = U.Get_resize_ratio(origin, shape)
        out["K_ratio"][i] = U.Create_K_resize(K.copy(), K.copy(), origin, origin, shape)[0][:3, :3]
        out["K_axes"][i] = U.scale_intrinsics(K.copy(), [float(w0) / w_t, float(h0) / h_t])
    path = os.path.join(REPO, "tests", "golden", "prepare_intrinsics.npz")
    np.savez_compressed(path, **out)
    print("%s: %d arrays, %d bytes" % (path, len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
