"""Command line of the track-indexed fingerprint library (grafp_amd/library.py).

  python -m grafp_amd.identify build --config CFG --ckp MODEL.pth --source DIR|JSON|FILES... --out LIBDIR [--precision]
  python -m grafp_amd.identify query --ckp MODEL.pth --library LIBDIR FILES... [--top 5] [--window S --hop S]

`build` fingerprints every track of the source (anything DeviceAudioCorpus accepts) into LIBDIR; `query` prints one JSON
object per query file -- or, with --window, one per timeline span of each file."""
import argparse
import json
import sys

import torch


def _model(cfg, ckp, device):
    from .train import build_model
    from .util import strip_module_prefix
    model = build_model(cfg, device=device)
    state = torch.load(ckp, map_location=device, weights_only=False)
    model.load_state_dict(strip_module_prefix(state["state_dict"] if "state_dict" in state else state))
    return model.eval()


def main(argv=None):
    from .util import DEFAULT_CONFIG, load_config
    ap = argparse.ArgumentParser(prog="python -m grafp_amd.identify", description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    b = sub.add_parser("build", help="fingerprint a corpus into a library directory")
    b.add_argument("--config", default=DEFAULT_CONFIG)
    b.add_argument("--ckp", required=True)
    b.add_argument("--source", required=True, nargs="+", help="a directory, the reference's JSON index, or files")
    b.add_argument("--out", required=True)
    b.add_argument("--precision", choices=("bf16", "f32"), default="bf16")
    b.add_argument("--max-segments", type=int, default=4096)
    q = sub.add_parser("query", help="identify recordings against a library")
    q.add_argument("--config", default=DEFAULT_CONFIG, help="model configuration (the library keeps its own "
                                                            "segmentation settings)")
    q.add_argument("--ckp", required=True)
    q.add_argument("--library", required=True)
    q.add_argument("files", nargs="+")
    q.add_argument("--top", type=int, default=5)
    q.add_argument("--k-probe", type=int, default=20)
    q.add_argument("--window", type=float, default=None, help="seconds per window: report a timeline per file")
    q.add_argument("--hop", type=float, default=1.0)
    q.add_argument("--force", action="store_true", help="use a library made with another model")
    args = ap.parse_args(argv)

    from .data import DeviceAudioCorpus
    from .library import FingerprintLibrary
    device = torch.device("cuda")
    cfg = load_config(args.config)
    model = _model(cfg, args.ckp, device)
    if args.cmd == "build":
        source = args.source[0] if len(args.source) == 1 else args.source
        corpus = DeviceAudioCorpus(cfg, source, device)
        lib = FingerprintLibrary.build(model, corpus, cfg, precision=args.precision, max_segments=args.max_segments)
        lib.save(args.out)
        print(json.dumps({"library": args.out, "tracks": lib.n_tracks, "rows": lib.n_rows}))
        return 0
    lib = FingerprintLibrary.load(args.library, model, device, force=args.force)
    if args.window is None:
        for path, matches in zip(args.files, lib.identify(list(args.files), top=args.top, k_probe=args.k_probe)):
            print(json.dumps({"query": path, "matches": matches}))
    else:
        for path in args.files:
            windows = lib.identify_windows(path, window_s=args.window, hop_s=args.hop, top=args.top,
                                           k_probe=args.k_probe)
            for span in lib.timeline(windows):
                print(json.dumps({"query": path, **span}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
