"""Every entry point of train.hip (include/vtc_hip.h, "adapter-only training step") against a float64 reference of the same
operation, one test per primitive: vtc_transpose_f32, vtc_colsum_f32, vtc_layernorm_bwd, vtc_attention_small_bwd, vtc_quickgelu,
vtc_normalize_rows_bwd, vtc_clip_loss_bwd, vtc_adam_step, vtc_axpby, vtc_scale_rows -- at the shapes AdapterTrainer.step never
calls them with (widths off the 64-lane grid, row counts off the 4-rows-per-workgroup grid, L from 1 to 16, accumulate_dx 0,
amsgrad 0, y given, group 6) -- and the composed step at B = 7, nc = 3 (Bp = 32, L = 4: the K = 32 GEMM).

References, case lists and the row-scaled error measure e = max |got - ref64| / scale: tests/primitive_refs.py.

The CPU half (no `gpu` mark) runs over the SAME case lists: it calibrates every tolerance (TOL below = 4 x the worst e of the
float32 torch evaluation, asserted to stay within TOL / 4 so that a drifting case list cannot outgrow the constant) and proves
that each deliberately wrong reference of an op exceeds the tolerance on at least one case.

Findings of these tests on the commit that introduced them (fixed with it):
  * vtc_adam_step formed its bias corrections in float, 1 - powf(beta, step): p missed its tolerance at steps 2 .. 5
    (e = 3.3e-6 against 1.15e-6; the cancellation keeps powf's half ulp near 1, up to 7e-6 relative in 1 - beta2^t).  They are
    formed in double now, as torch.optim does.
"""
import pytest
import torch

import primitive_refs as PR

torch.set_grad_enabled(False)
gpu = pytest.mark.gpu

# op -> output -> tolerance = 4 x (worst e of torch float32, on one CPU thread, over the op's cases: the figure in the comment), rounded up
TOL = {
    "layernorm_bwd": {"dx": 9.7e-7,          # 2.410e-07
                      "dgamma": 6.2e-7,      # 1.529e-07
                      "dbeta": 9.0e-7},      # 2.234e-07
    "attention_small_bwd": {"dqkv": 3.0e-6},  # 7.252e-07
    "normalize_rows_bwd": {"dx": 7.1e-7},    # 1.759e-07
    "clip_loss_bwd": {"dsim": 1.55e-6,       # 3.789e-07
                      "row_sums": 6.8e-7,    # 1.676e-07
                      "col_sums": 6.9e-7},   # 1.723e-07
    "quickgelu": {"y": 5.3e-7,               # 1.324e-07
                  "dx": 3.9e-6},             # 9.595e-07
    "adam_step": {"p": 1.15e-6,             # 2.818e-07
                  "m": 4.5e-7,               # 1.121e-07
                  "v": 6.1e-7,               # 1.511e-07
                  "vmax": 6.1e-7},           # 1.511e-07
    "colsum_f32": {"out": 4.6e-7},           # 1.139e-07
    # no rounding freedom on exactly representable data: equality
    "transpose_f32": {"y": 0.0}, "axpby": {"out": 0.0}, "scale_rows": {"x": 0.0},
}
# the composed step, B = 7, nc = 3: worst row-scaled gradient error of the float32 oracle against the float64 oracle over the two
# steps and both branches 1.011e-04 (step 2 of the image branch: a weight-gradient row whose largest entry is 1e-3 of the tensor's)
TOL_STEP = 4.1e-4


def _cases(name):
    return pytest.mark.parametrize("case", PR.OPS[name].cases, ids=lambda c: "-".join(str(v) for v in c))


def _ops():
    from vtc_amd import ops
    return ops


def _refused(match):
    return pytest.raises(RuntimeError, match=match)


# ==== CPU half: calibration and the proof that the tests can fail ========================================================================
def _worst_fp32(name):
    op = PR.OPS[name]
    if name != "adam_step":
        return op.calibrate()
    worst = {o: 0.0 for o in op.outs}
    for c in op.cases:                                           # the five-step sequence the GPU test walks
        with PR.single_thread():
            walked = PR.adam_walk(c, lambda inp: op.ref(inp, PR.F32))
        for o, v in walked.items():
            worst[o] = max(worst[o], v)
    return worst


def _worst_mutation(name, mut):
    op = PR.OPS[name]
    if name != "adam_step":
        return op.mutation_errors(mut)
    worst = {o: 0.0 for o in op.outs}
    for c in op.cases:
        for o, v in PR.adam_walk(c, lambda inp: op.ref(inp, PR.F64, mut)).items():
            worst[o] = max(worst[o], v)
    return worst


@pytest.mark.parametrize("name", PR.TRAIN_OPS)
def test_calibration_float32_stays_within_a_quarter_of_the_tolerance(name):
    worst = _worst_fp32(name)
    print(f"[calibration] {name}: " + "  ".join(f"{o} {v:.3e}" for o, v in worst.items()))
    for o, v in worst.items():
        assert v <= TOL[name][o] / 4, (name, o, v, TOL[name][o])


@pytest.mark.parametrize("name,mut", [(n, m) for n in PR.TRAIN_OPS for m in PR.OPS[n].muts])
def test_wrong_reference_exceeds_the_tolerance(name, mut):
    worst = _worst_mutation(name, mut)
    print(f"[mutation] {name} {mut}: " + "  ".join(f"{o} {v:.3e}" for o, v in worst.items()))
    assert any(v > TOL[name][o] for o, v in worst.items()), (name, mut, worst)


def test_adam_sequence_has_steps_whose_v_falls_below_vmax():
    """The data property the amsgrad case rests on: from step 3 on v < vmax for most elements, so a kernel that stored v would differ."""
    op = PR.OPS["adam_step"]
    state, grads = PR.adam_sequence((1000, 1))
    for t, g in enumerate(grads, start=1):
        out = op.ref({**state, "g": g, "step": t, "amsgrad": 1}, PR.F64)
        state = dict(zip(("p", "m", "v", "vmax"), out))
        if t >= 3:
            assert (state["v"] < state["vmax"]).float().mean() > 0.5
    assert (abs(grads[0]) < 1e-8 * 10).any() and (abs(grads[0]) > 0.1).any()          # both sides of eps


def _step_case(branch):
    from oracle import arch as A
    gen = torch.Generator().manual_seed(7)
    sd = {k: v for k, v in A.synth_model(A.VIT_B32, 61, "clip_finaltf").items()
          if k.startswith("final_transformer.") or k in ("mask_embedding", "model.logit_scale", "final_linear.weight")}
    B, nc, D = 7, 3, 512
    fv, ft = torch.randn(B, D, generator=gen), torch.randn(B, D, generator=gen)
    fc = torch.randn(nc, B, D, generator=gen)
    empty = torch.rand(B, nc, generator=gen) < 0.3
    skips = [torch.rand(B, generator=gen) > 0.5 for _ in range(2)]
    return sd, fv, ft, fc, empty, skips


def _oracle_step(sd, fv, ft, fc, empty, skip, branch, dtype):
    """One step of the oracle in `dtype` from the parameters `sd` -> (loss, gradients, parameters after its Adam step as fp32)."""
    from oracle import train_ref as TR
    sdd = {k: v.detach().cpu().to(dtype).clone() for k, v in sd.items()}
    opt = TR.AdamAmsgrad({k: sdd[k] for k in TR.adapter_param_names(sdd)})
    loss, grads = TR.train_step(fv.to(dtype), ft.to(dtype), fc.to(dtype), empty, skip, sdd, opt, branch=branch)
    return loss, grads, {k: v.float() for k, v in sdd.items()}


def _grad_error(got, ref64):
    """Row-scaled: a weight gradient [O, I] is judged row by row against the row's largest |ref64|, a vector as one row."""
    worst = {}
    for k, r in ref64.items():
        sc = r.abs().amax(-1, keepdim=True) if r.dim() == 2 else r.abs().max()
        worst[k] = PR.err(got[k].reshape(r.shape), r, sc)
    return worst


@pytest.mark.parametrize("branch", ["text", "image"])
def test_calibration_of_the_composed_step(branch):
    """Both steps of the GPU test: the float32 oracle against the float64 oracle from the same (fp32) parameters."""
    sd, fv, ft, fc, empty, skips = _step_case(branch)
    worst = 0.0
    for step, skip in enumerate(skips):
        _, g64, after = _oracle_step(sd, fv, ft, fc, empty, skip, branch, PR.F64)
        with PR.single_thread():
            _, g32, _ = _oracle_step(sd, fv, ft, fc, empty, skip, branch, PR.F32)
        worst = max(worst, max(_grad_error(g32, g64).values()))
        if step == 0:
            # a wrong step is seen: the empty-comment substitution of one token flipped
            empty2 = empty.clone()
            empty2[1, 1] = ~empty2[1, 1]
            _, gm, _ = _oracle_step(sd, fv, ft, fc, empty2, skip, branch, PR.F64)
            assert max(_grad_error(gm, g64).values()) > TOL_STEP
        sd = after
    print(f"[calibration] composed step {branch}: {worst:.3e}")
    assert worst <= TOL_STEP / 4


# ==== GPU half ===========================================================================================================================
def _run(name, inp, dev="cuda"):
    """The entry point of op `name` on the inputs of one case -> its outputs on the CPU, in the order of Op.outs.  Output buffers start
    from garbage: whatever the entry point must overwrite or zero, it must overwrite or zero itself."""
    ops = _ops()
    d = lambda k: inp[k].to(dev)                                  # noqa: E731
    if name == "layernorm_bwd":
        w = inp["x"].shape[1]
        dx, dg, db = d("dx0").clone(), torch.full((w,), 1e30, device=dev), torch.full((w,), -1e30, device=dev)
        ops.layernorm_bwd(d("x"), d("gamma"), d("dy"), dx=dx, accumulate_dx=bool(inp["accumulate_dx"]), dgamma=dg, dbeta=db)
        return dx.cpu(), dg.cpu(), db.cpu()
    if name == "attention_small_bwd":
        return (ops.attention_small_bwd(d("qkv"), d("dout"), inp["n_seq"], inp["L"], inp["heads"], out=d("dqkv0").clone()).cpu(),)
    if name == "normalize_rows_bwd":
        return (ops.normalize_rows_bwd(d("x"), d("dy"), out=d("dx0").clone()).cpu(),)
    if name == "clip_loss_bwd":
        return PR.clip_loss_bwd_sums(ops.clip_loss_bwd(d("sim"), out=d("dsim0").clone()).cpu())
    if name == "quickgelu":
        return ops.quickgelu(d("x"), out=d("out0").clone()).cpu(), ops.quickgelu(d("x"), d("dy"), out=d("out0").clone()).cpu()
    if name == "adam_step":
        h = PR.ADAM_HYPER                                         # unrounded, as a caller passes them: the ABI's float arguments round
        p, m, v, g = d("p").clone(), d("m").clone(), d("v").clone(), d("g")
        vmax = d("vmax").clone() if inp["amsgrad"] else None      # amsgrad = 0: vmax = NULL is accepted
        ops.adam_step(p, g, m, v, vmax, h["lr"], h["beta1"], h["beta2"], h["eps"], inp["step"], bool(inp["amsgrad"]))
        return p.cpu(), m.cpu(), v.cpu(), (vmax.cpu() if vmax is not None else inp["vmax"])
    if name == "colsum_f32":
        return (ops.colsum(d("x"), out=d("out0").clone()).cpu(),)
    if name == "transpose_f32":
        return (ops.transpose(d("x"), out=d("y0").clone()).cpu(),)
    if name == "axpby":
        x = d("x").clone()
        out = x if inp["alias"] else d("out0").clone()
        return (ops.axpby(x, d("y") if inp["y"] is not None else None, inp["a"], inp["b"], out=out).cpu(),)
    if name == "scale_rows":
        return (ops.scale_rows(d("x").clone(), d("s"), inp["group"]).cpu(),)
    raise KeyError(name)


def _check(name, case):
    op = PR.OPS[name]
    inp = op.make(case)
    got = _run(name, inp)
    op.check(inp, got, TOL[name], str(case))
    return inp, got


@gpu
@_cases("layernorm_bwd")
def test_layernorm_bwd(case):
    """dx with accumulate_dx 0 (over random data it must overwrite) and 1 (onto random data), dgamma / dbeta over buffers pre-filled
    with +-1e30 that the entry point must zero; widths 4 .. 1024 incl. 100 (lanes with different element counts), rows 1 .. 2310."""
    _check("layernorm_bwd", case)


@gpu
@pytest.mark.parametrize("width", [1028, 6])
def test_layernorm_bwd_refuses_unsupported_widths(width):
    ops = _ops()
    x = torch.zeros(3, width, device="cuda")
    dg, db = torch.full((width,), 5.0, device="cuda"), torch.full((width,), 5.0, device="cuda")
    with _refused(f"width={width}"):
        ops.layernorm_bwd(x, torch.ones(width, device="cuda"), x, dgamma=dg, dbeta=db)
    assert float(dg.min()) == 5.0 and float(db.min()) == 5.0      # nothing was launched, not even the zeroing


@gpu
@_cases("attention_small_bwd")
def test_attention_small_bwd(case):
    """All three thirds of dqkv, each (sequence, head) block against its own scale; L 1 .. 16, heads 1 .. 12, n_seq * heads on and
    off the 4-waves-per-workgroup grid, scores with a real spread and with one dominant key (exact zeros in P)."""
    inp, _ = _check("attention_small_bwd", case)
    if case[3] == "dominant":
        (q, k, _), _ = PR.split_qkv(inp, PR.F32)
        P = ((q @ k.transpose(-1, -2)) / 8).softmax(-1)
        assert inp["L"] == 1 or (P == 0).any()                    # the data property the case is named for


@gpu
@pytest.mark.parametrize("L_", [0, 17])
def test_attention_small_bwd_refuses_lengths_outside_1_to_16(L_):
    ops = _ops()
    qkv, dout = torch.zeros(2 * 17, 3 * 64, device="cuda"), torch.zeros(2 * 17, 64, device="cuda")
    out = torch.full_like(qkv, 5.0)
    with _refused(f"L={L_}"):
        ops.attention_small_bwd(qkv, dout, 2, L_, 1, out=out)
    assert float(out.min()) == 5.0


@gpu
@_cases("normalize_rows_bwd")
def test_normalize_rows_bwd(case):
    _check("normalize_rows_bwd", case)


@gpu
@_cases("clip_loss_bwd")
def test_clip_loss_bwd(case):
    """dsim entry by entry, and its row and column sums against the reference's (the structural check: see
    primitive_refs.clip_loss_bwd_sums for why they are not 0); n 1 .. 1000, logits at the model's scale and randn * 4."""
    _check("clip_loss_bwd", case)


@gpu
def test_clip_loss_bwd_refuses_a_small_workspace():
    ops = _ops()
    n = 65
    sim, out = torch.zeros(n, n, device="cuda"), torch.full((n, n), 5.0, device="cuda")
    with _refused("workspace too small"):
        ops.clip_loss_bwd(sim, out=out, ws=torch.zeros(4 * n - 1, device="cuda"))
    assert float(out.min()) == 5.0


@gpu
@_cases("quickgelu")
def test_quickgelu_forward_and_backward(case):
    inp, (y, dx) = _check("quickgelu", case)
    # the saturated tails are exact wherever float64 rounds to that: 0 / x forward, 0 / dy backward
    x, dy = inp["x"], inp["dy"]
    ry, rdx = (r.float() for r in PR.OPS["quickgelu"].ref(inp, PR.F64))
    tail = x.abs() >= 30
    for got, ref, ident in ((y, ry, x), (dx, rdx, dy)):
        zero, same = tail & (ref == 0), tail & (ref == ident)
        assert (got[zero] == 0).all() and torch.equal(got[same], ident[same])
    if case[1] != "rand":                                         # the data property: both tails are there, on either side
        assert (tail & (ry == x)).sum() > 50 and (tail & (rdx == dy)).sum() > 50
    if case[1] == "lin120":
        assert (tail & (ry == 0)).sum() > 50 and (tail & (rdx == 0)).sum() > 50


@gpu
@_cases("adam_step")
def test_adam_step_five_steps(case):
    """Five consecutive steps carrying the kernel's own state; p, m, v, vmax compared after every step, each step's reference starting
    from the state the kernel produced.  amsgrad 1: from step 3 on v falls below vmax and vmax must be kept; amsgrad 0: vmax = NULL."""
    worst = PR.adam_walk(case, lambda inp: _run("adam_step", inp))
    print(f"[e] adam_step {case}: " + "  ".join(f"{o} {v:.3e} (tol {TOL['adam_step'][o]:.1e})" for o, v in worst.items()))
    bad = {o: v for o, v in worst.items() if not v <= TOL["adam_step"][o]}
    assert not bad, (case, bad)


@gpu
def test_adam_step_refuses_amsgrad_without_vmax():
    ops = _ops()
    p = torch.full((300,), 5.0, device="cuda")
    z = torch.zeros(300, device="cuda")
    with _refused("amsgrad needs vmax"):
        ops.adam_step(p, torch.ones(300, device="cuda"), z, z.clone(), None, 1e-3, 0.9, 0.999, 1e-8, 1, True)
    assert float(p.min()) == 5.0


@gpu
@_cases("transpose_f32")
def test_transpose_f32(case):
    inp, (y,) = _check("transpose_f32", case)
    assert torch.equal(y, inp["x"].t())


@gpu
@_cases("colsum_f32")
def test_colsum_f32(case):
    """Rows above and below the 64-way row split, columns around the 256-thread workgroup; the output buffer starts from garbage.
    Integer data: every partial sum is exact in fp32, so the float atomics' order cannot matter -- equality."""
    inp, (out,) = _check("colsum_f32", case)
    if case[2] == "int":
        assert torch.equal(out, inp["x"].double().sum(0).float())


@gpu
@_cases("axpby")
def test_axpby(case):
    inp, (out,) = _check("axpby", case)
    assert torch.equal(out, PR.OPS["axpby"].ref(inp, PR.F64)[0].float())


@gpu
@_cases("scale_rows")
def test_scale_rows(case):
    inp, (x,) = _check("scale_rows", case)
    assert torch.equal(x, PR.OPS["scale_rows"].ref(inp, PR.F64)[0].float())


@gpu
@pytest.mark.parametrize("branch", ["text", "image"])
def test_train_step_full_width_small_batch_vs_fp64(branch):
    """The composed step of the full-width family (width 512, 8 heads, 2 layers) at B = 7, nc = 3: Bp = 32 and L = 4, so the batch
    is ONE K-step of the fp32 dgrad / wgrad GEMMs and the attention runs at L = 4.  Two steps; every gradient is judged row by row
    against the float64 oracle run from the trainer's own parameters of that step."""
    from vtc_amd.host.adapter_train import AdapterTrainer
    sd, fv, ft, fc, empty, skips = _step_case(branch)
    tr = AdapterTrainer({k: v.cuda() for k, v in sd.items()}, branch=branch)
    figures = []
    for step, skip in enumerate(skips):
        now = dict(sd)
        now.update({k: v.detach().cpu().clone() for k, v in tr.params.items()})
        ref_loss, g64, _ = _oracle_step(now, fv, ft, fc, empty, skip, branch, PR.F64)
        loss = float(tr.step(fv.cuda(), ft.cuda(), fc.cuda(), empty.cuda(), skip.cuda()).cpu())
        e = _grad_error({k: v.cpu() for k, v in tr.grads.items()}, g64)
        worst = max(e, key=e.get)
        print(f"[e] composed step {branch} step {step}: loss {loss:.7f} (ref {ref_loss:.7f})  worst {worst} {e[worst]:.3e} (tol {TOL_STEP:.1e})")
        figures.append((step, abs(loss - ref_loss), worst, e[worst]))
        assert set(g64) == set(tr.grads)
    for step, dl, worst, ev in figures:
        assert dl < 1e-5 * max(1.0, abs(ref_loss)) and ev <= TOL_STEP, (step, dl, worst, ev)
