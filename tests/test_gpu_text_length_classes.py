"""The ragged text tower at the sequence lengths where its attention core changes behaviour -- both sides of every 16-key tile
edge and of the 32 | 33 and 64 | 65 row boundaries a dispatch by length class would cut at (built in round 13 and taken out again:
not bit-identical at 384 sequences) -- with degenerate batches, and the one-pass entry of the embedding into the folded
(hi, lo) stream.

Every case runs the same ids through the host-offset entry point (vtc_text_forward_ragged), the device-offset one
(vtc_text_forward2, ragged) and the dense path: the two ragged paths must agree BIT FOR BIT (same rows, same tiles),
ragged against dense and against the fp32 oracle follows tests/test_gpu_towers.py::test_ragged_text_tower_equals_dense -- its rule
and its tolerance (`tol_for`, imported; that test's 1e-3 between ragged and dense is tol_for at its 512-d embedding, here taken at
the embedding width of the architecture in use).  As there, the oracle bound is asserted for the operand formats the product ships
(IEEE-half text blocks in bf16 mode, and fp32): with bf16 OPERANDS the rounding floor of the format itself is above it (max 1.1 -
1.4e-3 at 512-d with no kernel involved, `report_text` / tests/bf16_floor_study.py; test_text_tower_half_layers_statistics prints
that setting and asserts the shipped one), so that format's distance to the oracle is printed, and what is asserted for it is what
this file is about: the two ragged paths bit for bit, ragged against dense, independence of the order.  The architectures are oracle/arch.py's TINY text tower with the real context of
77 positions (TINY's own 24 never leave the first class), two blocks: the oracle takes a fraction of a second."""
from dataclasses import replace

import numpy as np
import pytest
import torch

from oracle import arch as A
from oracle import clip_ref as CR
from test_gpu_towers import cuda_sd, report_text, tol_for, unit

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TINY77 = replace(A.TINY, context_length=77)                                                   # 128 wide, 2 heads: the LayerNorm kernels
TINY77_H4 = replace(A.TINY, context_length=77, transformer_width=256, transformer_heads=4)    # 256 wide: the folded path
TINY77_W512 = replace(A.TINY, context_length=77, transformer_width=512, transformer_heads=8)
EDGES = [2, 3, 16, 17, 32, 33, 48, 64, 65, 77, 77, 2]       # rows per sequence (SOT and EOT included): both sides of every class edge
# operand formats of the 16-bit mode: the shipped one (every block on IEEE half) and bf16 operands; + fp32 (the same three launches)
FORMATS = [pytest.param(torch.bfloat16, None, id="half"), pytest.param(torch.bfloat16, 0, id="bf16"), pytest.param(torch.float32, None, id="f32")]


def ids_with_rows(rows, arch, seed):
    """[len(rows), ctx] token ids: SOT, rows[s] - 2 words, EOT, zero padding."""
    g = torch.Generator().manual_seed(seed)
    ids = torch.zeros(len(rows), arch.context_length, dtype=torch.int64)
    for s, r in enumerate(rows):
        assert 2 <= r <= arch.context_length
        ids[s, 0] = A.SOT
        ids[s, 1:r - 1] = torch.randint(1, A.SOT, (r - 2,), generator=g)
        ids[s, r - 1] = A.EOT
    return ids


_packed = {}


def packed(arch, wseed, dtype, half_layers):
    """one packed tower and one state dict per (architecture, format): shared by the cases, never modified"""
    from vtc_amd import towers
    key = (arch, wseed, dtype, half_layers)
    if key not in _packed:
        sd = A.synth_text(arch, wseed, prefix="model.")
        _packed[key] = (sd, towers.PackedText(cuda_sd(sd), "model.", dtype, heads=arch.transformer_heads, half_layers=half_layers))
    return _packed[key]


def check_paths(name, arch, sd, pt, ids, dtype, shipped_format=True):
    t = ids.cuda()
    host = pt.forward_host_offsets(t)
    dev = pt.forward(t, ragged=True)
    assert torch.isfinite(dev).all(), name
    assert torch.equal(dev, host), f"{name}: device-offset and host-offset ragged paths differ"
    ragged = dev.cpu().numpy()
    dense = pt.forward(t, ragged=False).cpu().numpy()
    ref = CR.encode_text(ids, sd, arch, "model.").numpy()
    if dtype == torch.float32:
        d = np.abs(ragged - dense).max()
        print(f"[parity] {name}: ragged - dense {d:.3e}; unit - oracle {np.abs(unit(ragged) - unit(ref)).max():.3e}")
        assert d < 2e-5 * np.abs(dense).max(), name
        assert np.abs(unit(ragged) - unit(ref)).max() < tol_for(dtype), name
    else:
        d = np.abs(unit(ragged) - unit(dense)).max()
        print(f"[parity] {name}: unit ragged - unit dense {d:.3e} (tol {tol_for(dtype, arch.embed_dim):.1e})")
        if shipped_format:
            report_text(name, unit(ragged), unit(ref), dtype, arch.embed_dim)
        else:
            print(f"[parity] {name}: bf16 operands, max abs err {np.abs(unit(ragged) - unit(ref)).max():.3e} (the format's floor: not asserted)")
        assert d < tol_for(dtype, arch.embed_dim), name
    return dev


@pytest.mark.parametrize("dtype,half_layers", FORMATS)
def test_class_edges_in_order_and_shuffled(dtype, half_layers):
    """Row counts on both sides of 32 | 33 and 64 | 65, the shortest and the longest sequence, two tiles' edges (16 | 17, 48), as
    listed and in one shuffled order: a sequence's feature does not depend on where in the batch it stands."""
    arch = TINY77
    sd, pt = packed(arch, 310, dtype, half_layers)
    ids = ids_with_rows(EDGES, arch, 311)
    out = check_paths(f"class edges {dtype}", arch, sd, pt, ids, dtype, half_layers is None)
    perm = torch.randperm(len(EDGES), generator=torch.Generator().manual_seed(312))
    assert not torch.equal(perm, torch.arange(len(EDGES)))
    out_p = check_paths(f"class edges, shuffled {dtype}", arch, sd, pt, ids[perm].contiguous(), dtype, half_layers is None)
    assert torch.equal(out_p, out[perm.cuda()]), "a sequence's feature changed with its place in the batch"


@pytest.mark.parametrize("dtype,half_layers", FORMATS)
@pytest.mark.parametrize("case", ["first_class_only", "last_class_only", "one_sequence", "five_sequences_4_heads", "five_sequences_2_heads"])
def test_degenerate_class_populations(case, dtype, half_layers):
    """Only short sequences, only full-length ones, a single sequence, and five sequences: with TINY's 2 heads five sequences fill
    the core's last workgroup (4 waves) half, with 4 heads every workgroup is one sequence."""
    arch, rows = {
        "first_class_only": (TINY77, [2, 32, 17, 5, 31, 9, 32]),
        "last_class_only": (TINY77, [77] * 6),
        "one_sequence": (TINY77, [40]),
        "five_sequences_4_heads": (TINY77_H4, [70, 3, 33, 64, 20]),
        "five_sequences_2_heads": (TINY77, [10, 12, 30, 2, 25]),
    }[case]
    sd, pt = packed(arch, 320, dtype, half_layers)
    check_paths(f"{case} {dtype}", arch, sd, pt, ids_with_rows(rows, arch, 321), dtype, half_layers is None)


@pytest.mark.parametrize("arch", [pytest.param(TINY77, id="W128"), pytest.param(TINY77_W512, id="W512")])
def test_text_entry_folded_and_unfolded(arch):
    """Nine ragged sequences with the fold on (W = 512: the embedding enters the (hi, lo) pair in one pass; W = 128 is below the
    fold's 256-column tiles and keeps the LayerNorm kernels either way) and with VTC_TOWER_NO_LN_FOLD (embedding to fp32, LayerNorm
    kernels): both hold the oracle, and each other, at the tower tolerance.  (Bit-identity of the one-pass entry with the two
    kernels it replaces is recorded against the parent build: profiles/r13_attention_cores.md.)"""
    from vtc_amd import towers
    dtype = torch.bfloat16
    sd = A.synth_text(arch, 330, prefix="model.")
    pt = towers.PackedText(cuda_sd(sd), "model.", dtype, heads=arch.transformer_heads)
    ids = ids_with_rows([2, 9, 77, 33, 64, 18, 65, 32, 50], arch, 331)
    ref = unit(CR.encode_text(ids, sd, arch, "model.").numpy())
    outs = {}
    for fold in (True, False):
        pt.w.flags = towers.tower_flags(ln_fold=fold)
        host = pt.forward_host_offsets(ids.cuda())
        dev = pt.forward(ids.cuda(), ragged=True)
        assert torch.equal(dev, host), f"fold={fold}: device-offset and host-offset ragged paths differ"
        outs[fold] = unit(dev.cpu().numpy())
        report_text(f"text entry W={arch.transformer_width} fold={fold}", outs[fold], ref, dtype, arch.embed_dim)
    d = np.abs(outs[True] - outs[False]).max()
    print(f"[parity] text entry W={arch.transformer_width}: folded - unfolded {d:.3e} (tol {tol_for(dtype, arch.embed_dim):.1e})")
    assert d < tol_for(dtype, arch.embed_dim)
