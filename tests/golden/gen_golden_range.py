"""Writes tests/golden/range_hw4_ref.npz: what the reference's own range_image_labeling and cluster_assignment
(Homework4/foreground_clustering_range.py:51-95, :124-133) return, run verbatim, on foreground subsets of its three KITTI scans and on a
few small synthetic images.  The fixture holds DATA only.

Runs on a CPU (numpy + scipy):   python tests/golden/gen_golden_range.py <reference root>
  <reference root>/Homework4/foreground_clustering_range.py    imported whole, with inert sys.modules stubs for open3d, matplotlib,
                                                               sklearn.cluster, bottleneck and mylib (none of them is used by the two functions)
  <reference root>/Homework4/test/{000077,000099,000111}.bin

The reference's pcd_to_range_image cannot run (:34, math.asin with two arguments), so the projection is project_ref of
tests/test_range_clustering.py; idx_image is built from its pixels the way :29 / :39 build it.  Foreground stand-in: z > -1.3 and the y gate
of pcd_preprocessing (-15 < y < 30), then every k-th point so that the file stays below the largest fixture of tests/golden.  Every point
with a pixel coordinate inside the rounding band (pcr.h) is removed (at most 1 % of a cloud, else the generator stops), an image with a pair
inside the band of theta is refused; the numbers removed are recorded.

Per case <name>: <name>_image (f64), <name>_params (phi, theta, nn_mode), <name>_ref_label (int32), <name>_counts (labels of the reference,
connected components, components the reference never seeded, their pixels, points removed from the input) and, for the clouds,
<name>_points (f32 n x 3) and <name>_ref_cluster (int32 n).
"""
import importlib.util
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZE_CAP = 833861                       # kat_kitti_q5.npz, the largest fixture so far


def load_restatement():
    spec = importlib.util.spec_from_file_location("t_range", os.path.join(os.path.dirname(HERE), "test_range_clustering.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference(root):
    for name in ("open3d", "matplotlib", "matplotlib.pyplot", "sklearn", "sklearn.cluster", "bottleneck", "mylib"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["sklearn.cluster"].spectral_clustering = None
    sys.modules["matplotlib"].pyplot = sys.modules["matplotlib.pyplot"]
    sys.modules["sklearn"].cluster = sys.modules["sklearn.cluster"]
    sys.path.insert(0, os.path.join(root, "Homework4"))
    import foreground_clustering_range as ref
    return ref


def idx_image_of(pix, shape):
    idx_image = np.empty(shape, dtype=object)
    for i, p in enumerate(pix):
        if p >= 0:
            r, c = divmod(int(p), shape[1])
            idx_image[r, c] = np.append(idx_image[r, c], i)
    return idx_image


def record(out, t, ref, name, image, params, points=None, pix=None, removed=0):
    phi, theta, nn = params
    mine, inband = t.label_ref(image, phi, theta, nn)
    if inband:
        raise SystemExit(f"{name}: {inband} pairs inside the rounding band of theta: refused")
    idx_image = idx_image_of(pix, image.shape) if pix is not None else None
    ref_label = ref.range_image_labeling(image, idx_image, None, phi, theta, nn)
    lab = ref_label >= 0
    left = (ref_label < 0) & (image > 0)
    n_comp = int(mine.max()) + 1 if (mine >= 0).any() else 0
    counts = [np.unique(ref_label[lab]).size, n_comp, np.unique(mine[left]).size, int(left.sum()), removed]
    out[name + "_image"] = image
    out[name + "_params"] = np.array([phi, theta, nn], np.float64)
    out[name + "_ref_label"] = ref_label.astype(np.int32)
    out[name + "_counts"] = np.array(counts, np.int64)
    if points is not None:
        out[name + "_points"] = points
        out[name + "_ref_cluster"] = ref.cluster_assignment(idx_image, ref_label, points.shape[0]).astype(np.int32)
    print(f"{name}: image {image.shape}, reference labels {counts[0]} of {counts[1]} components, {counts[2]} components ({counts[3]} pixels) "
          f"never seeded, {removed} points removed from the input")


def main(root):
    t = load_restatement()
    ref = load_reference(root)
    out, cases = {}, []
    for scan, (res, theta, nn), step in (("000077", (0.7, 30.0, 7), 5), ("000099", (0.7, 30.0, 7), 5), ("000111", (1.0, 20.0, 4), 6)):
        raw = np.fromfile(os.path.join(root, "Homework4", "test", scan + ".bin"), dtype=np.float32).reshape(-1, 4)[:, :3]
        fg = raw[(raw[:, 2] > -1.3) & (raw[:, 1] < 30) & (raw[:, 1] > -15)][::step]
        band = t.project_ref(fg, res)["band"]
        if band.sum() > 0.01 * fg.shape[0]:
            raise SystemExit(f"{scan}: {int(band.sum())} of {fg.shape[0]} points inside the band: more than 1 %")
        pts = np.ascontiguousarray(fg[~band])
        pr = t.project_ref(pts, res)
        assert not pr["band"].any()
        name = "kitti" + scan
        record(out, t, ref, name, pr["image"], (res, theta, nn), pts, pr["pix"], int(band.sum()))
        cases.append(name)
    rng = np.random.default_rng(4)
    for k, (rows, cols, nn, theta, fill) in enumerate(((12, 40, 3, 25.0, 0.5), (30, 64, 7, 30.0, 0.35), (1, 50, 2, 10.0, 0.7), (24, 9, 8, 15.0, 0.6),
                                                       (40, 33, 1, 35.0, 0.45))):
        name = f"synth{k}"
        record(out, t, ref, name, t.random_image(rng, rows, cols, fill), (0.7, theta, nn))
        cases.append(name)
    out["cases"] = np.array(cases)
    path = os.path.join(HERE, "range_hw4_ref.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(f"{path}: {size} bytes")
    if size > SIZE_CAP:
        raise SystemExit(f"the fixture is larger than the largest one under tests/golden ({SIZE_CAP} bytes): subsample further")


if __name__ == "__main__":
    main(sys.argv[1])
