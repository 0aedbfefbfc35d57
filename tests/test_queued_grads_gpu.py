"""Weight and bias gradients whose reductions are QUEUED during a backward pass (seld_linear.begin_batch /
flush_batch, opened by seld_graph.GraphedTrainStep around every backward pass) hold nothing until the flush.  A gradient
that any autograd node reads on its way to a parameter's ``.grad`` -- the permuted copy of the stems' projection weight
was one -- must therefore never be queued.

Poisoning makes that deterministic: ``seld_linear.tall_product`` and ``seld_linear.column_sum`` are wrapped, and an output
that has just been queued is filled with NaN before it is handed back.  ``flush_batch`` overwrites every element of a
queued output, so correct code is unaffected; code that reads early reads NaN (instead of whatever the caching allocator
left in a ``torch.empty`` block, which is often the previous, correct run's result).

Every way a weight reaches ``_Linear.apply`` is run at the smallest row count that queues (512 rows: two chunks) and
its leaf gradients are compared (1) batched + poisoned against unbatched, (2) against a float64 statement of the same
products and (3) for finiteness; the Conformer and ResNet50-Conformer run one eager iteration each way and three
captured ones at 3 x 250 frames (750 rows: two chunks for every width)."""
import pytest
import torch

from test_graph_gpu import _batches, _no_dropout

pytestmark = pytest.mark.gpu

ROWS = 512                       # chunk_count(512, <= 128, <= 128) == 2: the smallest row count that queues


class _Poison:
    """The wrappers described above; ``queued`` counts the outputs that were queued (and poisoned)."""

    def __init__(self, monkeypatch):
        import seld_linear
        self.queued = 0
        tall_product, column_sum = seld_linear.tall_product, seld_linear.column_sum

        def poisoned(kind, out):
            batch = seld_linear._batch
            if batch is not None and isinstance(out, torch.Tensor) and any(o is out for _, o in batch[kind]):
                out.fill_(float("nan"))
                self.queued += 1
            return out

        monkeypatch.setattr(seld_linear, "tall_product", lambda *a, **k: poisoned("sums", tall_product(*a, **k)))
        monkeypatch.setattr(seld_linear, "column_sum", lambda *a, **k: poisoned("cols", column_sum(*a, **k)))


def _half_ulp(dtype):
    """Relative: bf16 carries 8 significant bits (7 stored), fp32 24."""
    return 2.0 ** -8 if dtype == torch.bfloat16 else 2.0 ** -24


def _reference(x2, g2, w_dtype, b_dtype):
    """float64 dW = g2^T x2 and db = column sums of g2, from the operands AS THE KERNELS SEE THEM (x2 [N, K] and g2 [N, G]
    already in the compute dtype), with an elementwise error bound for what seld_linear computes:

      * the rows are split into ``chunks`` blocks; each block's product is a GEMM that accumulates in fp32 and rounds its
        result to the OPERANDS' dtype (the partial products of ``tall_chunks``):  half an ulp of that dtype on |P_c|
        (bf16: 2^-8 |P_c|; for fp32 operands this rounding is one more step of the fp32 chain below);
      * all N products of an output element and the ``chunks`` partial sums are added in fp32, in some order: at most
        N + chunks roundings of relative size 2^-24 each on partial sums that never exceed S = sum_r |g| |x|, whatever
        the order (the standard bound (n - 1) u sum|a_i b_i| for a recursive sum of n terms);
      * the result is rounded once to the leaf's dtype: half an ulp of it on |dW|.

    bound(dW) = 1.01 * (u_out |dW| + u_partial sum_c |P_c| + (N + chunks) 2^-24 S); the factor 1.01 covers the products
    of these first-order terms.  db is a plain fp32 column sum of N terms rounded to the bias dtype:
    bound(db) = 1.01 * (u_out |db| + N 2^-24 sum_r |g|)."""
    import seld_linear
    x, g = x2.detach().double().cpu(), g2.detach().double().cpu()
    n = x.shape[0]
    chunks = seld_linear.chunk_count(n, g.shape[1], x.shape[1])
    assert chunks > 1, "this shape would not queue"
    dw = g.t() @ x
    s = g.abs().t() @ x.abs()
    parts = sum((gc.t() @ xc).abs() for gc, xc in zip(g.chunk(chunks), x.chunk(chunks)))
    u_partial = _half_ulp(torch.bfloat16) if x2.dtype == torch.bfloat16 else 0.0
    w_bound = 1.01 * (_half_ulp(w_dtype) * dw.abs() + u_partial * parts + (n + chunks) * 2.0 ** -24 * s)
    db = g.sum(dim=0)
    b_bound = None if b_dtype is None else 1.01 * (_half_ulp(b_dtype) * db.abs() + n * 2.0 ** -24 * g.abs().sum(dim=0))
    return dw, w_bound, db, b_bound


# ---- the routes: each returns (leaves {name: parameter}, run() -> None (forward + backward), want() -> {name: (ref, bound)})

def _randn(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen) * scale


def _route_leaf(device, dtype, gen):
    from seld_linear import SeldLinear
    layer = SeldLinear(48, 24).to(device).to(dtype)
    x = _randn(gen, 2, ROWS // 2, 48).to(device).to(dtype)
    go = _randn(gen, 2, ROWS // 2, 24).to(device).to(dtype)

    def want():
        dw, wb, db, bb = _reference(x.reshape(ROWS, 48), go.reshape(ROWS, 24), dtype, dtype)
        return {"weight": (dw, wb), "bias": (db, bb)}
    return {"weight": layer.weight, "bias": layer.bias}, lambda: layer(x).backward(go), want


def _route_projection(c, f, out):
    def route(device, dtype, gen):
        from seld_linear import linear_on_channels_last_features
        layer = torch.nn.Linear(c * f, out).to(device).to(dtype)
        y = _randn(gen, 2, c, ROWS // 2, f).to(device).to(dtype).contiguous(memory_format=torch.channels_last)
        go = _randn(gen, 2, ROWS // 2, out).to(device).to(dtype)

        def run():
            got = linear_on_channels_last_features(layer, y)
            assert got is not None
            got.backward(go)

        def want():                                            # the reference's feature order: channel-major
            feats = y.permute(0, 2, 1, 3).reshape(ROWS, c * f)
            dw, wb, db, bb = _reference(feats, go.reshape(ROWS, out), dtype, dtype)
            return {"weight": (dw, wb), "bias": (db, bb)}
        return {"weight": layer.weight, "bias": layer.bias}, run, want
    return route


def _route_conv1x1(device, dtype, gen):
    import seld_linear
    c, o = 32, 48
    conv = torch.nn.Conv2d(c, o, 1, bias=False).to(device).to(dtype).to(memory_format=torch.channels_last)
    x = _randn(gen, 2, c, 16, 16).to(device).to(dtype).contiguous(memory_format=torch.channels_last)
    go = _randn(gen, 2, o, 16, 16).to(device).to(dtype).contiguous(memory_format=torch.channels_last)

    def run():
        y = seld_linear.conv1x1(conv, x)
        assert y.shape == go.shape and y.grad_fn is not None and "Convolution" not in type(y.grad_fn).__name__
        y.backward(go)

    def want():
        dw, wb, _, _ = _reference(x.permute(0, 2, 3, 1).reshape(ROWS, c), go.permute(0, 2, 3, 1).reshape(ROWS, o), dtype, None)
        return {"weight": (dw.view(o, c, 1, 1), wb.view(o, c, 1, 1))}
    return {"weight": conv.weight}, run, want


def _route_pointwise(d_in, d_out):
    """One of seld_dwconv.conv_module_forward's two pointwise calls: ``_Linear.apply(y, conv.weight.squeeze(-1), conv.bias)``."""
    def route(device, dtype, gen):
        from seld_linear import _Linear
        conv = torch.nn.Conv1d(d_in, d_out, kernel_size=1).to(device).to(dtype)
        x = _randn(gen, 2, ROWS // 2, d_in).to(device).to(dtype)
        go = _randn(gen, 2, ROWS // 2, d_out).to(device).to(dtype)

        def want():
            dw, wb, db, bb = _reference(x.reshape(ROWS, d_in), go.reshape(ROWS, d_out), dtype, dtype)
            return {"weight": (dw.unsqueeze(-1), wb.unsqueeze(-1)), "bias": (db, bb)}
        return ({"weight": conv.weight, "bias": conv.bias},
                lambda: _Linear.apply(x, conv.weight.squeeze(-1), conv.bias).backward(go), want)
    return route


def _route_qkv(device, dtype, gen):
    from model_conformer import MultiHeadSelfAttention
    d, heads = 16, 4
    attn = MultiHeadSelfAttention(d, heads).to(device).to(dtype)
    attn.pack_parameters()
    x = _randn(gen, 2, ROWS // 2, d).to(device).to(dtype)
    go = _randn(gen, 3, 2, heads, ROWS // 2, d // heads).to(device).to(dtype)          # for stack(q, k, v), each [B, H, T, Dh]
    leaves = {}
    for name in ("w_q", "w_k", "w_v"):
        leaves[f"{name}.weight"], leaves[f"{name}.bias"] = getattr(attn, name).weight, getattr(attn, name).bias

    def run():
        import seld_pack
        assert seld_pack.adjacent(attn.w_q.weight, attn.w_k.weight, attn.w_v.weight)
        torch.stack(attn._qkv(x)).backward(go)

    def want():                                                # _Linear's output columns are ordered (q|k|v, head, dim)
        g2 = go.permute(1, 3, 0, 2, 4).reshape(ROWS, 3 * d)
        dw, wb, db, bb = _reference(x.reshape(ROWS, d), g2, dtype, dtype)
        out = {}
        for i, name in enumerate(("w_q", "w_k", "w_v")):
            rows = slice(i * d, (i + 1) * d)
            out[f"{name}.weight"], out[f"{name}.bias"] = (dw[rows], wb[rows]), (db[rows], bb[rows])
        return out
    return leaves, run, want


def _route_twin(kind):
    """A non-leaf weight (or bias) of another kind than the projection's: a COPY whose backward node reads the gradient."""
    def route(device, dtype, gen):
        from seld_linear import _Linear
        layer = torch.nn.Linear(40, 24).to(device).to(dtype)
        perm = torch.randperm(40, generator=gen).to(device)
        x = _randn(gen, ROWS, 40).to(device).to(dtype)
        go = _randn(gen, ROWS, 24).to(device).to(dtype)

        def run():
            w, b = layer.weight, layer.bias
            if kind == "scaled":
                w = w * 1.0
            elif kind == "indexed":
                w = w[:, perm]
            else:
                b = b * 1.0
            _Linear.apply(x, w, b).backward(go)

        def want():
            dw, wb, db, bb = _reference(x, go, dtype, dtype)
            if kind == "indexed":                              # d leaf[:, perm[j]] = dW[:, j]
                inverse = torch.argsort(perm.cpu())
                dw, wb = dw[:, inverse], wb[:, inverse]
            return {"weight": (dw, wb), "bias": (db, bb)}
        return {"weight": layer.weight, "bias": layer.bias}, run, want
    return route


ROUTES = {
    "leaf": _route_leaf,
    "projection_c8_f4": _route_projection(8, 4, 16),           # [2, 8, 256, 4] with nn.Linear(32, 16)
    "projection_c16_f3": _route_projection(16, 3, 24),         # C != F, F odd: the column-mapped reduction
    "projection_c6_f5": _route_projection(6, 5, 16),           # C != F, F odd, outside that kernel's shapes
    "conv1x1": _route_conv1x1,
    "pointwise1": _route_pointwise(32, 64),
    "pointwise2": _route_pointwise(32, 32),
    "qkv": _route_qkv,
}
TWINS = {"scaled": _route_twin("scaled"), "indexed": _route_twin("indexed"), "scaled_bias": _route_twin("scaled_bias")}


def _three_checks(route, device, dtype, monkeypatch):
    import seld_linear
    from seld_linear import SeldLinear
    torch.manual_seed(0)
    gen = torch.Generator().manual_seed(7)
    leaves, run, want = route(device, dtype, gen)
    side = SeldLinear(16, 16).to(device).to(dtype)             # a leaf Linear in the same backward pass: always queued
    side_x, side_go = _randn(gen, ROWS, 16).to(device).to(dtype), _randn(gen, ROWS, 16).to(device).to(dtype)

    def grads(batched):
        for p in list(leaves.values()) + list(side.parameters()):
            p.grad = None
        if batched:
            seld_linear.begin_batch()
        try:
            run()
            side(side_x).backward(side_go)
        except BaseException:
            seld_linear.abandon_batch()
            raise
        if batched:
            assert seld_linear.flush_batch() == poison.queued
        return {k: p.grad.detach().clone() for k, p in leaves.items()}

    plain = grads(False)
    poison = _Poison(monkeypatch)
    queued = grads(True)
    assert seld_linear._batch is None
    assert poison.queued > 0, "nothing was queued: the case fell into the single-chunk path"
    expected = want()
    assert expected.keys() == leaves.keys()
    for name, p in leaves.items():
        a, b = plain[name], queued[name]
        assert a.dtype == p.dtype and a.shape == p.shape
        assert torch.isfinite(b.float()).all(), f"{name}: read before the flush filled it"              # (3)
        assert torch.isfinite(a.float()).all(), name
        if name.endswith("weight"):                                                                     # (1)
            assert torch.equal(a, b), name
        else:                                  # biases: the row blocks are added in a different fixed order
            assert (a.float() - b.float()).abs().max().item() <= 2.0 ** -7 * a.float().abs().max().item(), name
        ref, bound = expected[name]                                                                     # (2)
        for got in (a, b):
            err = (got.double().cpu() - ref).abs()
            worst = (err / bound.clamp_min(1e-300)).max().item()
            print(f"{name}: max error / bound = {worst:.3f}")
            assert (err <= bound).all(), (name, worst)
    return poison.queued


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(ROUTES))
def test_every_route_into_linear_survives_poisoned_queues(gpu_device, monkeypatch, name, dtype):
    _three_checks(ROUTES[name], gpu_device, dtype, monkeypatch)


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("name", list(TWINS))
def test_copied_weights_of_other_kinds_are_not_read_early(gpu_device, monkeypatch, name, dtype):
    """The rule, not the one call site: ``weight * 1.0``, ``weight[:, perm]`` and ``bias * 1.0`` are copies whose
    backward nodes read the returned gradient at once; the leaf parameter behind each must get the same gradient as
    without a batch."""
    _three_checks(TWINS[name], gpu_device, dtype, monkeypatch)


@pytest.mark.parametrize("name,count", [("leaf", 4), ("pointwise1", 4), ("qkv", 4), ("conv1x1", 3)])
def test_leaves_and_view_routes_still_queue_every_reduction(gpu_device, monkeypatch, name, count):
    """Leaves and the routes autograd passes through as views keep their place in the batched launches: the weight's and
    the bias's reduction of the route (conv1x1 has no bias) and of the leaf layer beside it."""
    assert _three_checks(ROUTES[name], gpu_device, torch.bfloat16, monkeypatch) == count


# ---- model level ---------------------------------------------------------------------------------------------------

def _stepper(kind, device, graphs):
    import seld_graph
    import trainer
    torch.manual_seed(0)
    model = _no_dropout(trainer.prepare_model_for_device(trainer.build_model((18, 36)), device)).train()
    trainer.enable_master_weights(model, device)
    crit = trainer.SMRSELDLoss("mse", 1.0, grid_size=(18, 36))
    opt = trainer.make_optimizer(model, 1e-3, device, capturable=True)
    step = seld_graph.GraphedTrainStep(model, crit, opt, device, autocast=lambda: trainer.autocast_context(device),
                                       use_graphs=graphs)
    return model, step


@pytest.mark.parametrize("kind", ["conformer", "resnet_conformer"])
def test_model_gradients_with_poisoned_queues(gpu_device, monkeypatch, kind):
    """One eager iteration of the stepper with the reductions batched (and poisoned) and one without, on the same data:
    every gradient finite, the projection weight's within the 2e-2 relative L2 that
    test_other_models_capture_and_track_the_eager_loop allows for the attention backward's atomics.  Then three
    captured iterations, poisoned inside the graph: finite losses and parameters.
    MIOpen's convolutions run in deterministic mode, as in test_crnn_graph_replay_is_bit_identical_to_the_eager_loop:
    with its default solvers two IDENTICAL unbatched runs of the ResNet50 encoder already differ by 2.1e-2 in this
    measure (measured: 2.115e-2, 1.921e-2), which would leave the 2e-2 to chance; in deterministic mode they are equal
    bit for bit and batched against unbatched differs by 1.6e-3 (ResNet50-Conformer) / 9.4e-4 (Conformer)."""
    import trainer
    cfg = trainer.config
    saved = cfg.MODEL_TYPE, torch.backends.cudnn.deterministic
    cfg.MODEL_TYPE = kind
    torch.backends.cudnn.deterministic = True
    x, m = _batches(gpu_device, 1, 3)[0]                     # 3 x 250 frames: 750 rows, two chunks for every width
    try:
        model, step = _stepper(kind, gpu_device, False)
        step.batch_reductions = False
        total = step(x, m)[0].clone()
        plain = {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}
        step.close()
        assert torch.isfinite(total) and "proj.weight" in plain

        poison = _Poison(monkeypatch)
        model, step = _stepper(kind, gpu_device, False)
        assert step.batch_reductions
        total = step(x, m)[0].clone()
        queued = {n: p.grad.detach().float().clone() for n, p in model.named_parameters() if p.grad is not None}
        step.close()
        assert poison.queued > 0 and torch.isfinite(total)
        assert queued.keys() == plain.keys()
        for n in plain:
            assert torch.isfinite(plain[n]).all(), n
            assert torch.isfinite(queued[n]).all(), f"{n}: read before the flush filled it"
        a, b = plain["proj.weight"], queued["proj.weight"]
        assert (a - b).norm().item() <= 2e-2 * a.norm().item()

        before = poison.queued
        model, step = _stepper(kind, gpu_device, True)
        losses = torch.stack([step(x, m)[0].clone() for _ in range(6)]).cpu()        # 3 eager warm-ups, capture, 3 replays
        stats = step.stats()
        step.close()
        assert stats["capture_error"] is None and stats["graphs"] == 1 and stats["replays"] == 3
        assert poison.queued > before
        assert torch.isfinite(losses).all(), losses
        for n, v in trainer.model_state_dict(model).items():
            assert torch.isfinite(v.float()).all(), n
    finally:
        cfg.MODEL_TYPE, torch.backends.cudnn.deterministic = saved
