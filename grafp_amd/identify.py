"""Command line of the track-indexed fingerprint library (grafp_amd/library.py).

  python -m grafp_amd.identify build --config CFG --ckp MODEL.pth --source DIR|JSON|FILES... --out LIBDIR [--precision]
                                       [--index flat|ivfpq|half --nlist 64 --pq-m 64 --nprobe 20 --train-rows 65536]
                                       [--row-stride D] [--shards N [--devices cuda:0,cuda:1]]
  python -m grafp_amd.identify query --ckp MODEL.pth --library LIBDIR FILES... [--top 5] [--window S --hop S]
                                       [--tempo X [--tempo-step G]] [--query-stride Q]
  python -m grafp_amd.identify dedup --ckp MODEL.pth --library LIBDIR [--min-overlap 3] [--coverage 0.9] [--json OUT]
                                       [--tempo X [--tempo-step G]]
  python -m grafp_amd.identify match --ckp MODEL.pth --library LIBDIR FILES... [--min-overlap 3] [--min-votes 4]
                                       [--min-score S] [--top 8] [--k-probe 20] [--json OUT]
                                       [--tempo X [--tempo-step G]]
  python -m grafp_amd.identify monitor --ckp MODEL.pth LIBDIR FILES... [--chunk-s 1.0] [--window 3 --hop 1] [--top 5]
                                       [--query-stride Q] [--tempo X [--tempo-step G] [--tempo-lock N]]

`build` fingerprints every track of the source (anything DeviceAudioCorpus accepts) into LIBDIR -- with --index ivfpq as
a compact library of IVF-PQ codes (about 150 bytes per row instead of 772; `query` works on either form, `dedup` needs
the flat one), with --index half as a half library of bf16 rows (260 bytes per row, nothing trained, the search exact
over the rows held; `query`, `match` and `monitor` load whichever form the directory holds, `dedup`, --tempo,
--query-stride above 1, --row-stride and --shards need the flat one); `query` prints one JSON
object per query file -- or, with --window, one per timeline span of each file; `dedup` prints one JSON object per pair
of tracks that share audio, then one per group of duplicates (--json also writes both to a file); `match` takes whole
recordings that are not in the library and prints one JSON object per (recording, library track) that share audio, with
the span and the coverage (either form of a library; --json also writes them to a file).  build --row-stride D keeps
every D-th fingerprint row of each track (a flat library of 772 / D bytes per original row; `query` works on it
unchanged, `dedup` and `match` need every row).  query --tempo X also searches recordings that play up to X (0.06: six
per cent) faster or slower than the catalogue (a flat library that keeps every row; every match and timeline span then
carries "tempo" next to its score; --tempo-step G spaces the ratios searched G / 256 apart).  match --tempo X does the
same for whole recordings -- a pitched DJ set, a sped-up re-upload -- on a flat library that keeps every row: every
printed match then also carries "tempo", "tempo_num" and "track_overlap_s" (--tempo-step defaults to 1).  dedup --tempo X
also finds the tracks of the library that share audio at another speed -- a sped-up re-release, a varispeed remaster --:
every printed pair then also carries "tempo", "tempo_num" and "b_overlap_s" (--tempo-step defaults to 1).  `monitor` treats every file as one live channel: it feeds them to a
StreamMonitor (grafp_amd/monitor.py) chunk by chunk, all channels per push, prints one JSON object per window as it
becomes due ({"channel", "file", start_s, end_s, segment_start_s, matches}) and, when the files end, one per timeline
span of each channel ({"channel", "file", "span": ...}).  build --shards N writes a sharded library
(grafp_amd/sharded.py: N flat shards over contiguous track ranges, shard s on the s-th of --devices, all on one device
without it); `query`, `match` and `monitor` load a directory that holds shards.json as one (--devices again says where
the shards go) and answer as the one-card library would; `dedup` across shards is not built.  query --query-stride Q and
monitor --query-stride Q embed only every Q-th segment of the recordings (1 / Q of the model's work; a flat library that
keeps every row, no --tempo) and align those (csrc/identify_stride.hip); what is printed keeps its form.  monitor --tempo X
follows channels that play up to X faster or slower than the catalogue (a flat library that keeps every row, sharded or
not; every match and timeline span then carries "tempo"); --tempo-lock N searches a channel whose last N windows agreed
over three ratios instead of the whole grid (csrc/identify_tempo_items.hip) and marks every window "locked" or not."""
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
    b.add_argument("--index", choices=("flat", "ivfpq", "half"), default="flat",
                   help="flat: f32 rows; ivfpq: a compact library of IVF-PQ codes; half: bf16 rows, 260 bytes a row")
    b.add_argument("--nlist", type=int, default=64, help="ivfpq: inverted lists")
    b.add_argument("--pq-m", type=int, default=64, choices=(16, 32, 64, 128), help="ivfpq: code bytes per row")
    b.add_argument("--nprobe", type=int, default=20, help="ivfpq: lists a query row probes")
    b.add_argument("--train-rows", type=int, default=65536, help="ivfpq: rows the quantiser is trained on")
    b.add_argument("--row-stride", type=int, default=1,
                   help="flat: keep every D-th fingerprint row of each track (1..32); queries stay dense")
    b.add_argument("--shards", type=int, default=None, help="flat: write a library of this many shards")
    b.add_argument("--devices", default=None, help="--shards: the shards' devices, comma-separated (cuda:0,cuda:1)")
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
    q.add_argument("--tempo", type=float, default=None,
                   help="also search recordings that play up to this fraction faster or slower (0.06: 0.94 to 1.06)")
    q.add_argument("--tempo-step", type=int, default=None, help="spacing of the ratios searched, in 1/256")
    q.add_argument("--query-stride", type=int, default=1,
                   help="embed every Q-th segment of a recording only (1 to 32; a flat library that keeps every row)")
    q.add_argument("--force", action="store_true", help="use a library made with another model")
    q.add_argument("--devices", default=None, help="a sharded library: its shards' devices, comma-separated")
    d = sub.add_parser("dedup", help="find tracks of a library that share audio")
    d.add_argument("--config", default=DEFAULT_CONFIG, help="model configuration (the library keeps its own "
                                                            "segmentation settings)")
    d.add_argument("--ckp", required=True)
    d.add_argument("--library", required=True)
    d.add_argument("--min-overlap", type=float, default=3.0, help="seconds of shared audio a pair needs")
    d.add_argument("--coverage", type=float, default=0.9, help="share of the shorter track that makes a duplicate")
    d.add_argument("--min-score", type=float, default=None, help="duplicate score bar (default: the library's)")
    d.add_argument("--k-probe", type=int, default=32)
    d.add_argument("--json", default=None, help="also write {pairs, groups} to this file")
    d.add_argument("--tempo", type=float, default=None,
                   help="also find tracks that share audio up to this fraction faster or slower (0.06: 0.94 to 1.06)")
    d.add_argument("--tempo-step", type=int, default=None, help="spacing of the ratios searched, in 1/256 (default 1)")
    d.add_argument("--force", action="store_true", help="use a library made with another model")
    m = sub.add_parser("match", help="find what whole recordings share with a library")
    m.add_argument("--config", default=DEFAULT_CONFIG, help="model configuration (the library keeps its own "
                                                            "segmentation settings)")
    m.add_argument("--ckp", required=True)
    m.add_argument("--library", required=True)
    m.add_argument("files", nargs="+")
    m.add_argument("--min-overlap", type=float, default=3.0, help="seconds of shared audio a match needs")
    m.add_argument("--min-votes", type=int, default=4, help="rows whose hits must agree on the alignment")
    m.add_argument("--min-score", type=float, default=None, help="drop weaker matches (default: keep all)")
    m.add_argument("--top", type=int, default=8, help="library tracks reported per recording")
    m.add_argument("--k-probe", type=int, default=20)
    m.add_argument("--json", default=None, help="also write the matches to this file")
    m.add_argument("--tempo", type=float, default=None,
                   help="also match recordings that play up to this fraction faster or slower (0.06: 0.94 to 1.06)")
    m.add_argument("--tempo-step", type=int, default=None, help="spacing of the ratios searched, in 1/256 (default 1)")
    m.add_argument("--force", action="store_true", help="use a library made with another model")
    m.add_argument("--devices", default=None, help="a sharded library: its shards' devices, comma-separated")
    mo = sub.add_parser("monitor", help="follow files as live channels, chunk by chunk")
    mo.add_argument("--config", default=DEFAULT_CONFIG, help="model configuration (the library keeps its own "
                                                             "segmentation settings)")
    mo.add_argument("--ckp", required=True)
    mo.add_argument("library", metavar="LIBDIR")
    mo.add_argument("files", nargs="+")
    mo.add_argument("--chunk-s", type=float, default=1.0, help="seconds of audio every channel gets per push")
    mo.add_argument("--window", type=float, default=3.0)
    mo.add_argument("--hop", type=float, default=1.0)
    mo.add_argument("--top", type=int, default=5)
    mo.add_argument("--k-probe", type=int, default=20)
    mo.add_argument("--min-score", type=float, default=None, help="timeline: drop windows whose best match is weaker")
    mo.add_argument("--query-stride", type=int, default=1,
                    help="embed every Q-th segment of a channel only (1 to 32; a flat library that keeps every row)")
    mo.add_argument("--tempo", type=float, default=None,
                    help="also follow channels that play up to this much faster or slower, e.g. 0.06 (a flat library)")
    mo.add_argument("--tempo-step", type=int, default=None, help="spacing of the ratios searched, in 1/256")
    mo.add_argument("--tempo-lock", type=int, default=0,
                    help="with --tempo: windows that must agree before a channel is searched over three ratios only")
    mo.add_argument("--force", action="store_true", help="use a library made with another model")
    mo.add_argument("--devices", default=None, help="a sharded library: its shards' devices, comma-separated")
    args = ap.parse_args(argv)

    from .data import DeviceAudioCorpus
    from .library import FingerprintLibrary
    from .sharded import ShardedFingerprintLibrary
    devices = args.devices.split(",") if getattr(args, "devices", None) else None
    device = torch.device(devices[0] if devices else "cuda")
    cfg = load_config(args.config)
    model = _model(cfg, args.ckp, device)
    if args.cmd == "build":
        source = args.source[0] if len(args.source) == 1 else args.source
        corpus = DeviceAudioCorpus(cfg, source, device)
        if args.shards is not None or devices:
            if args.index != "flat":
                sys.exit("build --shards needs --index flat: compact shards are not built" if args.index == "ivfpq" else
                         "build --shards needs --index flat: shards of the half form are not built")
            lib = ShardedFingerprintLibrary.build(model, corpus, cfg, n_shards=args.shards, devices=devices,
                                                  precision=args.precision, max_segments=args.max_segments,
                                                  row_stride=args.row_stride)
            lib.save(args.out)
            print(json.dumps({"library": args.out, "index": "flat", "shards": len(lib.shards),
                              "row_stride": lib.row_stride, "tracks": lib.n_tracks, "rows": lib.n_rows,
                              "rows_per_shard": [sh.n_rows for sh in lib.shards], "bytes": lib.nbytes}))
            return 0
        lib = FingerprintLibrary.build(model, corpus, cfg, precision=args.precision, max_segments=args.max_segments,
                                       index=args.index, nlist=args.nlist, pq_m=args.pq_m, nprobe=args.nprobe,
                                       train_rows=args.train_rows, row_stride=args.row_stride)
        lib.save(args.out)
        stride = {"row_stride": lib.row_stride} if lib.row_stride != 1 else {}
        print(json.dumps({"library": args.out, "index": args.index, **stride, "tracks": lib.n_tracks,
                          "rows": lib.n_rows, "bytes": lib.nbytes}))
        return 0
    if ShardedFingerprintLibrary.is_sharded_dir(args.library):
        if args.cmd == "dedup":
            sys.exit(f"{args.library}: dedup across the shards of a sharded library is not built "
                     "(ShardedFingerprintLibrary.self_matches)")
        lib = ShardedFingerprintLibrary.load(args.library, model, devices, force=args.force)
    else:
        lib = FingerprintLibrary.load(args.library, model, device, force=args.force)
    if args.cmd in ("dedup", "match") and lib.row_stride != 1:
        sys.exit(f"{args.library}: {args.cmd} needs every row of a track: this library keeps every {lib.row_stride}th "
                 f"(row_stride={lib.row_stride})")
    if args.cmd == "dedup":
        from .library import DUPLICATE_MIN_SCORE
        if getattr(lib, "is_half", False):
            sys.exit(f"{args.library}: dedup needs the flat form of a library (f32 rows): this one is of the half form "
                     "and holds bf16 rows only; build it with --index flat")
        if lib.is_compact:
            sys.exit(f"{args.library}: dedup needs the flat form of a library (f32 rows): this one is compact and holds "
                     "IVF-PQ codes only")
        pairs = lib.self_matches(k_probe=args.k_probe, min_overlap_s=args.min_overlap, tempo=args.tempo,
                                 tempo_step=args.tempo_step)
        bar = DUPLICATE_MIN_SCORE if args.min_score is None else args.min_score
        groups = [{"tracks": g, "names": [lib.names[t] for t in g]}
                  for g in lib.duplicate_groups(pairs, min_coverage=args.coverage, min_score=bar)]
        for p in pairs:
            print(json.dumps({"pair": p}))
        for g in groups:
            print(json.dumps({"group": g}))
        if args.json:
            with open(args.json, "w") as f:
                json.dump({"pairs": pairs, "groups": groups}, f, indent=1)
        return 0
    if args.cmd == "monitor":
        from .monitor import StreamMonitor
        waves = lib._load_queries(list(args.files), None)
        chunk = max(1, int(args.chunk_s * lib.settings["fs"]))
        mon = StreamMonitor(lib, len(waves), window_s=args.window, hop_s=args.hop, top=args.top, k_probe=args.k_probe,
                            max_chunk_s=args.chunk_s, query_stride=args.query_stride, tempo=args.tempo,
                            tempo_step=args.tempo_step, tempo_lock=args.tempo_lock)

        def report(per_channel):
            for ch, windows in enumerate(per_channel):
                for w in windows:
                    print(json.dumps({"file": args.files[ch], **w}), flush=True)

        for lo in range(0, max(w.numel() for w in waves), chunk):
            report(mon.push([w[lo:lo + chunk] for w in waves]))
            report(mon.end([ch for ch, w in enumerate(waves) if lo < w.numel() <= lo + chunk]))
        report(mon.end(range(len(waves))))                      # (empty files)
        for ch, path in enumerate(args.files):
            for span in mon.timeline(ch, args.min_score):
                print(json.dumps({"channel": ch, "file": path, "span": span}))
        return 0
    if args.cmd == "match":
        res = lib.match(list(args.files), k_probe=args.k_probe, min_overlap_s=args.min_overlap,
                        min_votes=args.min_votes, min_score=args.min_score, top=args.top, tempo=args.tempo,
                        tempo_step=args.tempo_step)
        found = [{"recording": path, **hit} for path, hits in zip(args.files, res) for hit in hits]
        for hit in found:
            print(json.dumps(hit))
        if args.json:
            with open(args.json, "w") as f:
                json.dump({"matches": found}, f, indent=1)
        return 0
    if args.window is None:
        for path, matches in zip(args.files, lib.identify(list(args.files), top=args.top, k_probe=args.k_probe,
                                                            tempo=args.tempo, tempo_step=args.tempo_step,
                                                            query_stride=args.query_stride)):
            print(json.dumps({"query": path, "matches": matches}))
    else:
        for path in args.files:
            windows = lib.identify_windows(path, window_s=args.window, hop_s=args.hop, top=args.top,
                                           k_probe=args.k_probe, tempo=args.tempo, tempo_step=args.tempo_step,
                                           query_stride=args.query_stride)
            for span in lib.timeline(windows):
                print(json.dumps({"query": path, **span}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
