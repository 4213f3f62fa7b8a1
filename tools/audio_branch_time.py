"""What the audio branch adds to a forward: the audio config's model (PretrainedCLIP_finaltf, ViT-B/32, init_audio_model=True,
branch text, 5 comments + 5 clips per item) against the SAME model and inputs without the audio (init_audio_model=False, 5 comments),
ms per forward timed with hip events, interleaved rounds, median.

    python tools/audio_branch_time.py [--batches 1,50,256] [--reps 20] [--rounds 5] [--dtype bf16|f16|f32] [--mlp]

--mlp also times the feature-MLP kernel alone at B * 5 rows.  Random weights (no checkpoint is needed to time).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--batches", default="1,50,256")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--dtype", default="bf16")
    ap.add_argument("--mlp", action="store_true")
    args = ap.parse_args()
    from oracle import arch as A
    from vtc_amd.host import model as HM
    torch.set_grad_enabled(False)
    torch.manual_seed(0)
    dtype = HM.parse_compute_dtype(args.dtype)
    audio = HM.PretrainedCLIP_finaltf(model_type="ViT-B/32", init_audio_model=True, audio_model_ckpt="", clip_audio_ckpt="")
    sd = audio.state_dict()
    plain = HM.PretrainedCLIP_finaltf(model_type="ViT-B/32")
    plain.load_state_dict({k: v for k, v in sd.items() if not k.startswith("audio_model.")}, strict=True)
    models = {}
    for name, m in (("audio", audio), ("no_audio", plain)):
        m = m.eval().cuda()
        m.compute_dtype = dtype
        models[name] = m
    rows = []
    for B in [int(b) for b in args.batches.split(",")]:
        vis = torch.randn(B, 3, 224, 224, device="cuda")
        title = A.synth_tokens(B, A.VIT_B32, 1).cuda()
        comments = A.synth_tokens(B * 5, A.VIT_B32, 2, empty_frac=0.1).reshape(B, 5, -1).cuda()
        clips = torch.randn(B, 5, 512, device="cuda")
        calls = {"audio": lambda: models["audio"](vis, title, [comments, clips]),
                 "no_audio": lambda: models["no_audio"](vis, title, comments)}
        if args.mlp:
            mlp = models["audio"]._pack()["audio"]
            x = clips.reshape(-1, 512)
            calls["mlp_only"] = lambda: mlp.forward(x)
        for f in calls.values():          # warm-up: packing, workspaces, first-call calibration
            f()
            f()
        torch.cuda.synchronize()
        times = {k: [] for k in calls}
        for _ in range(args.rounds):
            for k, f in calls.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(args.reps):
                    f()
                t1.record()
                t1.synchronize()
                times[k].append(t0.elapsed_time(t1) / args.reps)
        for m in models.values():
            m.check_finite()
        med = {k: statistics.median(v) for k, v in times.items()}
        row = {"B": B, "ms_audio": round(med["audio"], 4), "ms_no_audio": round(med["no_audio"], 4),
               "added_pct": round(100.0 * (med["audio"] / med["no_audio"] - 1.0), 2)}
        if "mlp_only" in med:
            row["ms_mlp_only"] = round(med["mlp_only"], 4)
        rows.append(row)
    print(f"{'B':>5} {'audio ms':>10} {'no audio ms':>12} {'added':>8}" + (f" {'MLP ms':>8}" if args.mlp else ""))
    for r in rows:
        print(f"{r['B']:>5} {r['ms_audio']:>10.3f} {r['ms_no_audio']:>12.3f} {r['added_pct']:>7.2f}%"
              + (f" {r['ms_mlp_only']:>8.4f}" if args.mlp else ""))
    print(json.dumps({"dtype": args.dtype, "rows": rows}))


if __name__ == "__main__":
    main()
