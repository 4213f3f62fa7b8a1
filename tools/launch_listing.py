"""The launch sequence and the output of one forward, over the smallest shapes that reach every branch of towers.hip: what a host-side
refactor of the tower orchestration must leave exactly as it was.

    python tools/launch_listing.py OUTDIR            # OUTDIR/listing.txt (class, region, work, tag per launch) + OUTDIR/<case>.npy
    python tools/launch_listing.py --compare A B     # listings line for line, outputs bit for bit (CPU)

Run the first form on both commits (same card), then compare the two directories."""
import ctypes as C
import os
import sys
from dataclasses import replace

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def compare(da, db):
    la, lb = (open(os.path.join(d, "listing.txt")).read().splitlines() for d in (da, db))
    bad = [i for i, (x, y) in enumerate(zip(la, lb)) if x != y]
    print(f"listing: {len(la)} / {len(lb)} lines, {len(bad)} differ" + (f" (first: line {bad[0] + 1}: {la[bad[0]]!r} | {lb[bad[0]]!r})" if bad else ""))
    names = sorted(f for f in os.listdir(da) if f.endswith(".npy"))
    diff = [f for f in names if not np.array_equal(np.load(os.path.join(da, f)), np.load(os.path.join(db, f)), equal_nan=True)]
    nonfinite = [f for f in names if not np.isfinite(np.load(os.path.join(da, f))).all()]
    print(f"outputs: {len(names)} cases, {len(diff)} not bit-identical {diff[:5]}, {len(nonfinite)} with a non-finite value")
    same_set = names == sorted(f for f in os.listdir(db) if f.endswith(".npy"))
    sys.exit(0 if (la == lb and not diff and not nonfinite and same_set) else 1)


def main(out_dir):
    import torch
    from oracle import arch as A
    from vtc_amd import _lib as L
    from vtc_amd import ops, towers
    torch.set_grad_enabled(False)
    os.makedirs(out_dir, exist_ok=True)
    lib, listing, max_rec = L.lib(), [], 4096

    def case(name, fn):
        lib.vtc_prof_begin()
        out = fn()
        n = C.c_int(0)
        cls, reg, tag = (C.c_int * max_rec)(), (C.c_int * max_rec)(), (C.c_int * (3 * max_rec))()
        ms, work = (C.c_double * max_rec)(), (C.c_double * max_rec)()
        L.check(lib.vtc_prof_end_records(ops._stream(), max_rec, C.byref(n), cls, reg, ms, work, tag), "vtc_prof_end_records")
        listing.append(f"== {name}: {n.value} launches")
        listing.extend(f"{L.PROF_CLASSES[cls[i]]} {L.PROF_REGIONS[reg[i]]} {work[i]!r} {tag[3 * i]} {tag[3 * i + 1]} {tag[3 * i + 2]}" for i in range(n.value))
        np.save(os.path.join(out_dir, name + ".npy"), out.cpu().numpy())

    cuda = lambda sd: {k: v.cuda() for k, v in sd.items()}
    a = replace(A.TINY, vision_width=256, transformer_width=256, transformer_heads=4)      # width 256: the LayerNorms fold; 2 layers
    wide = replace(A.TINY, vision_width=768)                                              # c_proj K = 3072: split-K
    sds = {"alt": A.synth_visual(a, 11, nframes=4, prefix="v."), "v1": A.synth_visual(a, 12, nframes=4, prefix="v.", variant="v1"),
           "img": A.synth_visual(a, 13, prefix="v."), "wide": A.synth_visual(wide, 14, prefix="v.")}
    sd_txt = A.synth_text(a, 15, prefix="t.")
    flag_sets = {"default": {}, "full": dict(full_last_layer=True), "nofold": dict(ln_fold=False), "nosplitk": dict(splitk=False)}
    dtypes = {"fp32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}
    for dn, dtype in dtypes.items():
        vis = {k: towers.PackedVision(cuda(sd), "v.", dtype) for k, sd in sds.items()}
        texts = {"": towers.PackedText(cuda(sd_txt), "t.", dtype, heads=a.transformer_heads)}
        if dtype == torch.bfloat16:      # all-bf16 blocks, and an operand-format boundary between block 0 and block 1
            texts.update({f"_half{h}": towers.PackedText(cuda(sd_txt), "t.", dtype, heads=a.transformer_heads, half_layers=h) for h in (0, 1)})
        for fn_, kw in flag_sets.items():
            for pk in list(vis.values()) + list(texts.values()):
                pk.w.flags = towers.tower_flags(**kw)
            for n in (1, 3):
                vid = A.synth_pixels((n, 4, 3, 64, 64), 20 + n).cuda()
                img = A.synth_pixels((n, 3, 64, 64), 30 + n).cuda()
                ids = A.synth_tokens(n + 2, a, 40 + n, empty_frac=0.2).cuda()
                for k in ("alt", "v1"):
                    case(f"{k}_{dn}_{fn_}_n{n}", lambda: vis[k].forward(vid))
                case(f"img_{dn}_{fn_}_n{n}", lambda: vis["img"].forward(img))
                if n == 1:
                    case(f"wide_{dn}_{fn_}_n{n}", lambda: vis["wide"].forward(img))
                for tn, pt in texts.items():
                    case(f"txt{tn}_ragged_{dn}_{fn_}_n{n}", lambda: pt.forward(ids[:n], ragged=True))
                    case(f"txt{tn}_dense_{dn}_{fn_}_n{n}", lambda: pt.forward(ids[:n], ragged=False))
                    case(f"txt{tn}_two_{dn}_{fn_}_n{n}", lambda: pt.forward(ids[:n], ragged=True, ids_b=ids[n:]))
                    case(f"txt{tn}_host_{dn}_{fn_}_n{n}", lambda: pt.forward_host_offsets(ids[:n]))
    # the CAM (fp32 / bf16 are its formats): nc = 5 comments, with and without 2 aux rows, one launch and many
    ca = replace(A.TINY, embed_dim=128)
    sd_cam, g = A.synth_cam(ca, 51), torch.Generator().manual_seed(52)
    for dn in ("fp32", "bf16"):
        cam = towers.PackedCam(cuda(sd_cam), dtypes[dn], 2, False, None)
        for B in (1, 3):
            main, comm, aux = (torch.randn(B * m, 128, generator=g).cuda() for m in (1, 5, 2))
            comments = A.synth_tokens(B * 5, ca, 53 + B, empty_frac=0.3).reshape(B, 5, -1).cuda()
            for fused in (None, False):
                case(f"cam_{dn}_B{B}_fused{fused}", lambda: cam.forward(main, comm, comments, fused=fused))
                case(f"cam_aux_{dn}_B{B}_fused{fused}", lambda: cam.forward(main, comm, comments, fused=fused, aux=aux))
    open(os.path.join(out_dir, "listing.txt"), "w").write("\n".join(listing) + "\n")
    print(f"{sum(1 for x in listing if x.startswith('=='))} cases, {len(listing)} lines -> {out_dir}")


if __name__ == "__main__":
    compare(*sys.argv[2:4]) if sys.argv[1] == "--compare" else main(sys.argv[1])
