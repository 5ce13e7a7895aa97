"""Score Ref-DAVIS / DAVIS-2017 label maps: J&F-Mean and the other global measures of the reference's eval_davis.py.

Reads the folder layout the reference's DAVIS / Results classes read (davis2017/davis.py, results.py):
    <davis_root>/ImageSets/2017/<subset>.txt                                   one sequence name per line
    <davis_root>/Annotations_unsupervised/<resolution>/<seq>/<frame>.png       ('Annotations' for the semi-supervised task)
    <results_path>/<seq>/<frame>.png                                           what inference.write_label_maps wrote
decodes the indexed PNGs with PIL, uploads each sequence once and scores it with one jf_counts call (one HIP kernel on the GPU,
the torch composition on the CPU), and writes global_results-<subset>.csv and per-sequence_results-<subset>.csv into results_path
with the reference's columns and %.5f.  Unlike the reference it does not need JPEGImages, and it always recomputes: CSVs of an
earlier run are overwritten, not read back.

    python -m ocpg_amd.eval_davis --results_path RESULTS [--davis_path ROOT] [--set val] [--task unsupervised]
"""
import argparse
import glob
import math
import os
import time

import numpy as np
import torch
from PIL import Image

from .metrics import GLOBAL_MEASURES, DavisAccumulator, davis_sequence_jf

TASKS = ("semi-supervised", "unsupervised")
DEFAULT_DAVIS_PATH = "../datasets/refer_davis/valid"


def _read_label_map(path):
    a = np.array(Image.open(path))
    if a.ndim != 2:
        raise ValueError(f"{path}: expected an indexed (palette or grey) PNG, got an array of shape {a.shape}")
    if a.max() > 255:
        raise ValueError(f"{path}: label {a.max()} does not fit a byte")
    return a.astype(np.uint8)


def sequence_names(davis_root, task="unsupervised", subset="val"):
    year = "2019" if task == "unsupervised" and subset in ("test-dev", "test-challenge") else "2017"          # davis.py:34
    path = os.path.join(davis_root, "ImageSets", year, f"{subset}.txt")
    if not os.path.exists(path):
        raise FileNotFoundError(f"sequence list {path} not found")
    with open(path) as f:
        return [x.strip() for x in f if x.strip()]


def read_sequence(davis_root, results_path, seq, task="unsupervised", resolution="480p"):
    """-> uint8 [2, T, H, W]: the ground-truth label maps of the sequence and the result label maps of the same frames."""
    folder = "Annotations" if task == "semi-supervised" else "Annotations_unsupervised"
    masks = sorted(glob.glob(os.path.join(davis_root, folder, resolution, seq, "*.png")))
    if not masks:
        raise FileNotFoundError(f"no annotations for sequence {seq} under {os.path.join(davis_root, folder, resolution)}")
    gt, res = [], []
    for m in masks:
        frame = os.path.splitext(os.path.basename(m))[0]
        r = os.path.join(results_path, seq, f"{frame}.png")
        if not os.path.exists(r):
            raise FileNotFoundError(f"{seq} frame {frame} not found: the results have to be indexed PNG files inside the sequence's folder")
        gt.append(_read_label_map(m))
        res.append(_read_label_map(r))
        if res[-1].shape != gt[0].shape or gt[-1].shape != gt[0].shape:
            raise ValueError(f"{seq} frame {frame}: annotation {gt[-1].shape} and result {res[-1].shape} must both be {gt[0].shape}")
    return np.stack([np.stack(gt), np.stack(res)])


def _fmt(x):
    return "" if math.isnan(x) else "%.5f" % x


def write_csvs(results_path, subset, global_results, per_object):
    g = os.path.join(results_path, f"global_results-{subset}.csv")
    with open(g, "w") as f:
        f.write(",".join(GLOBAL_MEASURES) + "\n")
        f.write(",".join(_fmt(global_results[k]) for k in GLOBAL_MEASURES) + "\n")
    s = os.path.join(results_path, f"per-sequence_results-{subset}.csv")
    with open(s, "w") as f:
        f.write("Sequence,J-Mean,F-Mean\n")
        for name, (jm, fm) in per_object.items():
            f.write(f"{name},{_fmt(jm)},{_fmt(fm)}\n")
    return g, s


def evaluate_davis(davis_root, results_path, task="unsupervised", subset="val", resolution="480p", device=None, write_csv=True):
    """-> ({measure: value} over GLOBAL_MEASURES, {'<seq>_<i>': (J mean, F mean)}); device None = the GPU when there is one."""
    if task not in TASKS:
        raise ValueError(f"The only tasks that are supported are {TASKS}")
    if device is None:
        device = "cuda" if torch.cuda.is_available() else "cpu"
    acc = DavisAccumulator()
    for seq in sequence_names(davis_root, task, subset):
        maps = torch.from_numpy(read_sequence(davis_root, results_path, seq, task, resolution)).to(device)
        j, f = davis_sequence_jf(maps[0], maps[1], task)
        acc.add(seq, j, f)
    global_results, per_object = acc.summary()
    if write_csv:
        write_csvs(results_path, subset, global_results, per_object)
    return global_results, per_object


def main(argv=None):
    ap = argparse.ArgumentParser(description="DAVIS-2017 J&F evaluation of a results folder")
    ap.add_argument("--davis_path", type=str, default=DEFAULT_DAVIS_PATH,
                    help="DAVIS folder containing ImageSets and Annotations / Annotations_unsupervised")
    ap.add_argument("--set", type=str, default="val", help="Subset to evaluate the results")
    ap.add_argument("--task", type=str, default="unsupervised", choices=list(TASKS), help="Task to evaluate the results")
    ap.add_argument("--results_path", type=str, required=True, help="Folder containing the sequences' folders")
    args, _ = ap.parse_known_args(argv)
    t0 = time.time()
    print(f"Evaluating sequences for the {args.task} task...")
    g, per = evaluate_davis(args.davis_path, args.results_path, task=args.task, subset=args.set)
    print(f"--------------------------- Global results for {args.set} ---------------------------")
    print(" ".join("%9s" % k for k in GLOBAL_MEASURES))
    print(" ".join("%9s" % _fmt(g[k]) for k in GLOBAL_MEASURES))
    print(f"\n---------- Per sequence results for {args.set} ----------")
    print("%-24s %8s %8s" % ("Sequence", "J-Mean", "F-Mean"))
    for name, (jm, fm) in per.items():
        print("%-24s %8s %8s" % (name, _fmt(jm), _fmt(fm)))
    print("\nTotal time: %.1f s" % (time.time() - t0))


if __name__ == "__main__":
    main()
