"""A/B of the training step with speed or time-stretch augmentation off and on (graph replay and eager), alternating
child processes:
    python tools/step_aug_ab.py PAIRS[,PAIRS...] [--aug speed|stretch] [--tree OTHER_CHECKOUT] [--both] [reps]
Each child builds the model from the same seed and times 20 steps after warm-up, as tools/step_lib_ab.py does; the parent
alternates the variants so that box drift hits all alike.  Variants: `off` (the shipped configuration: no augmentation
keys), `on` (--aug's keys, default speed: {aug}_prob = 1, {aug}_range = [0.94, 1.06]: every clip resampled or stretched,
views of draw_len samples), with --both also `both` (the other augmentation's keys on top: stretch, then speed), and with
--tree the `off` step of another built checkout of this repository (e.g. the parent commit), to show that off adds
nothing."""
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
AUGS = ("speed", "stretch")


def child(root, variant, pairs_list, aug):
    import torch
    sys.path.insert(0, root)
    from grafp_amd.train import Trainer, build_model, synthetic_batch
    from grafp_amd.util import load_config
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    for pairs in pairs_list:
        cfg = load_config()
        cfg["bsz_train"] = pairs
        for a in {"on": (aug,), "both": AUGS}.get(variant, ()):
            cfg.update({f"{a}_prob": 1.0, f"{a}_range": [0.94, 1.06]})
        torch.manual_seed(1234)
        model = build_model(cfg, device=dev)
        tr = Trainer(cfg, model, dev, amp_dtype=torch.bfloat16)
        x_i, x_j = synthetic_batch(pairs, 7, dev, n_samples=getattr(tr, "draw_len", None) or 16000)
        out = []
        for name, step in (("graph", tr.step_graph), ("eager", tr.step)):
            for _ in range(4):
                loss = step(x_i, x_j)
            torch.cuda.synchronize()
            best = 1e9
            for _ in range(3):
                t0 = time.perf_counter()
                for _ in range(20):
                    loss = step(x_i, x_j)
                torch.cuda.synchronize()
                best = min(best, (time.perf_counter() - t0) / 20 * 1e3)
            out.append(f"{name} {best:8.3f} ms")
        print(f"pairs={pairs:5d} {variant:6s}: " + "  ".join(out) + f"  loss {float(loss):.5f}", flush=True)
        del tr, model
        torch.cuda.empty_cache()


def main():
    if sys.argv[1] == "--child":
        return child(sys.argv[2], sys.argv[3], [int(v) for v in sys.argv[4].split(",")], sys.argv[5])
    args = sys.argv[1:]
    tree, aug = None, "speed"
    if "--tree" in args:
        i = args.index("--tree")
        tree = os.path.abspath(args[i + 1])
        del args[i:i + 2]
    if "--aug" in args:
        i = args.index("--aug")
        aug = args[i + 1]
        del args[i:i + 2]
    if aug not in AUGS:
        sys.exit(f"--aug {aug}: one of {AUGS}")
    both = "--both" in args
    if both:
        args.remove("--both")
    pairs, reps = args[0], int(args[1]) if len(args) > 1 else 3
    here = os.path.dirname(HERE)
    variants = ([(tree, "other")] if tree else []) + [(here, "off"), (here, "on")] + ([(here, "both")] if both else [])
    for _ in range(reps):
        for root, variant in variants:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", root, variant, pairs, aug], check=True)


if __name__ == "__main__":
    main()
