"""Fixture generator for Points, EuclideanTransformPoints and PostProcess — runs ONLY in the build container against the
real reference (mounted read-only at /root/reference; it never travels).

Writes
  points_golden.npz / points_golden_meta.json   transform chains (state, cloud, labels or exception type), to_image
                                                grids (np.packbits) or exception types, PostProcess fields on a reduced
                                                grid, and the example scripts' arrays on their reduced grid;
  image_pixels.npz                              the decoded pixels of the three test images (uint8), from which the
                                                tests rebuild image_clouds.npz with Points.from_image.
Every script builder of tests/points_scenes.py is first proven equal, bit for bit, to the script itself (executed with
plotting stubbed, as generate_example_golden.py does) on the script's own grid.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/generate_points_golden.py
"""
import json
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, "/root/reference/Code/spomso")
sys.dont_write_bytecode = True
IMAGES = "/root/reference/Files/test_images"

import spomso.cores as ref  # noqa: E402  (the real reference)
import points_scenes as S  # noqa: E402
from generate_example_golden import run_script  # noqa: E402


def chains(arrays, meta):
    out = {}
    for i, (name, points, steps) in enumerate(S.CHAINS):
        p, err = S.run_chain(ref, points, steps)
        rec = {"error": err, "labels": list(p.transformations) if p is not None else None}
        if p is not None:
            for attr in S.STATE:
                v = getattr(p, attr)
                rec[attr + "_type"] = type(v).__name__
                arrays["chain_%s_%s" % (name, attr)] = np.asarray(v)
            if err is None:
                try:
                    arrays["chain_%s_cloud" % name] = np.asarray(p.cloud)
                    rec["cloud_error"] = None
                except Exception as exc:  # noqa: BLE001
                    rec["cloud_error"] = type(exc).__name__
        out[name] = rec
    meta["chains"] = out


def to_image(arrays, meta):
    out = {}
    for case in S.TO_IMAGE:
        grid, err = S.to_image_case(ref, case)
        rec = {"error": err}
        if grid is not None:
            assert grid.dtype == np.float64 and set(np.unique(grid)) <= {0.0, 1.0}
            rec["shape"] = list(grid.shape)
            rec["occupied"] = int(np.count_nonzero(grid))
            arrays["image_%s" % case[0]] = np.packbits(grid.astype(bool).ravel())
        out[case[0]] = rec
    meta["to_image"] = out


def post_process(arrays, meta):
    co, res = ref.generate_grid(S.PP_SIZE, S.PP_RES)
    co = S.f32(co)
    out = {"grid": [list(S.PP_SIZE), list(S.PP_RES), [int(r) for r in res]]}
    for label, method, args in S.pp_methods(S.PP_RES):
        field, pp = S.pp_field(ref, method, args, co)
        arrays["pp_%s" % label] = np.asarray(field)
        out[label] = {"labels": list(pp.post_processing_operations), "shape": list(np.shape(field))}
    field, pp = S.pp_chain_field(ref, co)
    arrays["pp_chain"] = np.asarray(field)
    out["chain"] = {"labels": list(pp.post_processing_operations), "shape": list(np.shape(field))}
    meta["post_process"] = out


def scripts(arrays, meta):
    out = {}
    for path, (size, res), builder, names in S.SCRIPTS:
        space = run_script(path, {})
        co, _ = ref.generate_grid(size, res)
        mine = builder(ref, co)
        for var, key in names.items():
            want = mine if key is None else mine[key]
            assert np.array_equal(np.asarray(space[var]), np.asarray(want)), (path, var)      # builder IS the script
        co_small, _ = ref.generate_grid(size, S.SCRIPT_SMALL_RES)
        small = builder(ref, S.f32(co_small))
        stem = os.path.splitext(os.path.basename(path))[0]
        for var, key in names.items():
            arrays["script_%s_%s" % (stem, var)] = np.asarray(small if key is None else small[key])
        out[stem] = {"script": path, "grid": [list(size), list(S.SCRIPT_SMALL_RES)], "vars": sorted(names)}
    meta["scripts"] = out


def pixels():
    out = {"lines": np.asarray(Image.open(os.path.join(IMAGES, "lines_test_handdrawn.png")).convert("L")),
           "owl": np.asarray(Image.open(os.path.join(IMAGES, "owl_logo.png")).convert("LA")),
           "shapes": np.asarray(Image.open(os.path.join(IMAGES, "dilation_erosion.png")).convert("LA"))}
    np.savez_compressed(os.path.join(HERE, "image_pixels.npz"), **out)


def main():
    arrays, meta = {}, {}
    chains(arrays, meta)
    to_image(arrays, meta)
    post_process(arrays, meta)
    scripts(arrays, meta)
    np.savez_compressed(os.path.join(HERE, "points_golden.npz"), **arrays)
    with open(os.path.join(HERE, "points_golden_meta.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    pixels()
    for name in ("points_golden.npz", "points_golden_meta.json", "image_pixels.npz"):
        print("%-26s %8d bytes" % (name, os.path.getsize(os.path.join(HERE, name))))


if __name__ == "__main__":
    main()
