"""Step-level A/B of the fp16 few-row Linear / neck split-K kernels (OCPG_SMALL_LINEAR_FP16, OCPG_SPLITK_3X3_FP16): bench.py lines with
both switches on ("on": the default) and off ("off": the library path), alternated in ONE call so that both legs see the same machine.

    python tools/bench_small_linear_fp16.py --config c5 --rounds 3 --out profiles/small_linear_fp16_bench_lines.jsonl
    python tools/bench_small_linear_fp16.py --config r101 --rounds 3 --out ...
    python tools/bench_small_linear_fp16.py --config bf16 --rounds 3 --other /path/to/parent/checkout --out ...

c5: BASELINE config #5 (Video-Swin-B + RoBERTa, fp16, 8 x 480 x 854, 1 clip); r101: `--dtype fp16` with ResNet-101; bf16: the default
(bf16) line of this checkout against the same command in another checkout (`--other`: the parent commit, built), no switch set.
Every leg is a fresh child process (one GPU process at a time); its JSON line gets a "leg" key and is appended to --out, followed by a
summary line with ms_per_step per leg and the launches per step of the _h16 symbols where the `kernels` rows show them."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COMMON = ["--gpus", "1", "--no-cpu-baseline", "--no-b1"]
CONFIGS = {
    "c5": ["--backbone", "video_swin_b_p4w7", "--dtype", "fp16", "--text", "roberta", "--frames", "8", "--height", "480", "--width", "854",
           "--clips-per-gpu", "1"],
    "r101": ["--dtype", "fp16"],
    "bf16": [],
}
SWITCHES = ("OCPG_SMALL_LINEAR_FP16", "OCPG_SPLITK_3X3_FP16")


def run(root, argv, env_extra, timeout):
    env = dict(os.environ)
    for k in SWITCHES:
        env.pop(k, None)
    env.update(env_extra)
    p = subprocess.run([sys.executable, os.path.join(root, "bench.py")] + argv, cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    if p.returncode != 0 or not lines:
        sys.stderr.write(p.stderr[-2000:])
        raise SystemExit(f"bench.py failed (exit {p.returncode})")
    return json.loads(lines[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", choices=sorted(CONFIGS), required=True)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--kernel-timing", action="store_true", help="keep bench.py's per-kernel rows (extra eager steps per leg)")
    ap.add_argument("--other", default=None, help="bf16: the checkout to compare against (built)")
    ap.add_argument("--reverse", action="store_true", help="second leg first (off / parent), to see an order effect")
    ap.add_argument("--only", default=None, help="run one leg only (e.g. `on` with --kernel-timing for the launch counts)")
    ap.add_argument("--timeout", type=int, default=500)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    argv = COMMON + CONFIGS[a.config] + ["--steps", str(a.steps), "--warmup", str(a.warmup)] + ([] if a.kernel_timing else ["--no-kernel-timing"])
    if a.config == "bf16":
        if not a.other:
            raise SystemExit("--config bf16 needs --other")
        legs = [("branch", ROOT, {}), ("parent", os.path.abspath(a.other), {})]
    else:
        legs = [("on", ROOT, {}), ("off", ROOT, {k: "0" for k in SWITCHES})]
    if a.reverse:
        legs.reverse()
    if a.only:
        legs = [leg for leg in legs if leg[0] == a.only]
    ms = {name: [] for name, _, _ in legs}
    launches = {}
    for r in range(a.rounds):
        for name, root, env in legs:
            line = run(root, argv, env, a.timeout)
            line["leg"] = f"{a.config}_{name}_{r + 1}"
            ms[name].append(line["ms_per_step"])
            for row in line.get("kernels", []):
                if row["kernel"].endswith("_h16") and ("small_linear" in row["kernel"] or "splitk" in row["kernel"]):
                    launches.setdefault(name, {})[row["kernel"]] = row["launches_per_step"]
            print(f"{line['leg']}: {line['ms_per_step']:.3f} ms/step, launch {line['config'].get('launch')}, final_loss {line.get('final_loss')}", flush=True)
            if a.out:
                with open(a.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
    summary = {"summary": a.config, "ms_per_step": ms, "h16_launches_per_step": launches}
    print(json.dumps(summary), flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(json.dumps(summary) + "\n")


if __name__ == "__main__":
    main()
