"""`torch.ops.fitgnn.*`: the C-ABI launchers as schema-registered PyTorch custom ops (north_star: "exposed
as PyTorch-ROCm custom ops").  Importing this module registers

    fitgnn::spmm_csr(rowptr, col, val, X, tiles, window_rows, bias?, epilogue, p, seed, mask?) -> Y
    fitgnn::spmm_csr_t(... of the TRANSPOSED pattern ...)          the adjoint, used as spmm_csr's backward
    fitgnn::gcn_norm_csr(rowptr, col, w?) -> (val, dinv)
    fitgnn::epilogue_bwd(dOut, out, epilogue, p, seed, mask?) -> (dZ, db)
    fitgnn::pool_rows(assign, cval, n, X) -> Xc
    fitgnn::variation_costs(rowptr, col, w?, dw, A, set_off, set_mem) -> cost
    fitgnn::lift_adjacency(rowptr, col, w, assign, cval, n) -> (rowptr_c, col_c, w_c)
    fitgnn::gemm_nt(a, b) -> a @ b^T          fitgnn::gemm_atb(a, b) -> a^T @ b      (3 x bf16 MFMA kernels, fp32 in/out)
    fitgnn::linear(x, W) -> x @ W^T           differentiable: dX = gemm_nt(dY, W^T), dW = gemm_atb(dY, x)
    fitgnn::gcn_query_gather(rowptr, col, val, T, rows, xrow?, b0?) -> G      the two node-query launches (fitgnn_amd.serve)
    fitgnn::gcn_query_tail(G, W1, b1?, Wl, bl?, log_softmax) -> out
    fitgnn::gat_query_gather(rowptr, col, T, a_src0, a_dst0, u_src, u_dst, rows, xrow?, b0?, slope0, slope1) -> G     its GAT counterpart
    fitgnn::sage_query_gather(rowptr, col, val, T, rows, xrow?, b0?) -> G [Q, 2H] = [g_q | h_q]     its SAGE counterpart (T [n_table, 2H], the mean CSR)
    fitgnn::gin_query_hops(rowptr, col, val, T, eps0, W0b, b0b?, eps1, rows, xrow?, b0a?) -> G [Q, Hb]     the GIN pair (T [n_table, Ha], the sum CSR,
    fitgnn::gin_query_tail(G, W1a, b1a?, W1b, b1b?, Wl, bl?, log_softmax) -> out                           eps0 / eps1 one float each on the device)
    fitgnn::gcn_graph_query_hops(rowptr, col, val, T, seg, prow, pptr, max_rows, xrow?, b0?) -> G [P, H]     the two graph-query launches
    fitgnn::gcn_graph_query_tail(G, pptr, W1, b1?, Wl, bl?, pool (0 max, 1 mean), softmax) -> out [Q, C]     (fitgnn_amd.serve.GraphQueryEngine)
    fitgnn::gin_graph_query_hops(rowptr, col, val, T, eps0, W0b, b0b?, eps1, seg, prow, pptr, max_rows, xrow?, b0a?) -> G [P, Hb]     their GIN
    fitgnn::gin_graph_query_tail(G, pptr, W1a, b1a?, W1b, b1b?, Wl, bl?, pool (0 max, 1 mean), softmax) -> out [Q, C]                 counterparts
    fitgnn::gat_graph_query_hops(rowptr, col, T, a_src0, a_dst0, u_src, u_dst, seg, prow, pptr, max_rows, xrow?, b0?, slope0, slope1) -> G [P, H]     the GAT first launch (then gcn_graph_query_tail)
    fitgnn::sage_graph_query_hops(rowptr, col, val, T, seg, prow, pptr, max_rows, xrow?, b0?) -> G [P, 2H] = [g_r | h_r]     the SAGE first launch (T [n_table, 2H], the mean CSR; then gcn_graph_query_tail with K = 2H)
                                              (rows: int64 union rows inside the CSR -- not checked here, the kernel cannot; serve.QueryEngine checks)

for the CUDA (HIP) dispatch key only -- there is no CPU kernel, a CPU tensor fails in the dispatcher -- with fake
(meta) kernels for shape inference and an autograd formula for spmm_csr over a pair of forward / transposed
patterns.  The higher-level autograd Functions of fitgnn_amd.ops (fused layers) call the same launchers directly.
"""
import torch

from . import _lib, coarsening, ops

_LIB = torch.library.Library("fitgnn", "DEF")
_LIB.define("spmm_csr(Tensor rowptr, Tensor col, Tensor val, Tensor X, Tensor tiles, int window_rows, Tensor? bias, "
            "int epilogue, float p, int seed, Tensor? mask) -> Tensor")
_LIB.define("spmm_csr_pair(Tensor rowptr, Tensor col, Tensor val, Tensor tiles, Tensor rowptr_t, Tensor col_t, Tensor val_t, "
            "Tensor tiles_t, Tensor X, int window_rows) -> Tensor")
_LIB.define("gcn_norm_csr(Tensor rowptr, Tensor col, Tensor? w) -> (Tensor, Tensor)")
_LIB.define("epilogue_bwd(Tensor dOut, Tensor out, int epilogue, float p, int seed, Tensor? mask) -> (Tensor, Tensor)")
_LIB.define("pool_rows(Tensor assign, Tensor cval, int n, Tensor X) -> Tensor")
_LIB.define("variation_costs(Tensor rowptr, Tensor col, Tensor? w, Tensor dw, Tensor A, Tensor set_off, Tensor set_mem) -> Tensor")
_LIB.define("lift_adjacency(Tensor rowptr, Tensor col, Tensor w, Tensor assign, Tensor cval, int n) -> (Tensor, Tensor, Tensor)")
_LIB.define("gemm_nt(Tensor a, Tensor b) -> Tensor")
_LIB.define("gemm_atb(Tensor a, Tensor b) -> Tensor")
_LIB.define("linear(Tensor x, Tensor W) -> Tensor")
_LIB.define("gcn_query_gather(Tensor rowptr, Tensor col, Tensor val, Tensor T, Tensor rows, Tensor? xrow, Tensor? b0) -> Tensor")
_LIB.define("gat_query_gather(Tensor rowptr, Tensor col, Tensor T, Tensor a_src0, Tensor a_dst0, Tensor u_src, Tensor u_dst, Tensor rows, "
            "Tensor? xrow, Tensor? b0, float slope0, float slope1) -> Tensor")
_LIB.define("sage_query_gather(Tensor rowptr, Tensor col, Tensor val, Tensor T, Tensor rows, Tensor? xrow, Tensor? b0) -> Tensor")
_LIB.define("gin_query_hops(Tensor rowptr, Tensor col, Tensor val, Tensor T, Tensor eps0, Tensor W0b, Tensor? b0b, Tensor eps1, Tensor rows, "
            "Tensor? xrow, Tensor? b0a) -> Tensor")
_LIB.define("gin_query_tail(Tensor G, Tensor W1a, Tensor? b1a, Tensor W1b, Tensor? b1b, Tensor Wl, Tensor? bl, bool log_softmax) -> Tensor")
_LIB.define("gcn_query_tail(Tensor G, Tensor W1, Tensor? b1, Tensor Wl, Tensor? bl, bool log_softmax) -> Tensor")
_LIB.define("gcn_graph_query_hops(Tensor rowptr, Tensor col, Tensor val, Tensor T, Tensor seg, Tensor prow, Tensor pptr, int max_rows, "
            "Tensor? xrow, Tensor? b0) -> Tensor")
_LIB.define("gcn_graph_query_tail(Tensor G, Tensor pptr, Tensor W1, Tensor? b1, Tensor Wl, Tensor? bl, int pool, bool softmax) -> Tensor")
_LIB.define("gin_graph_query_hops(Tensor rowptr, Tensor col, Tensor val, Tensor T, Tensor eps0, Tensor W0b, Tensor? b0b, Tensor eps1, "
            "Tensor seg, Tensor prow, Tensor pptr, int max_rows, Tensor? xrow, Tensor? b0a) -> Tensor")
_LIB.define("gat_graph_query_hops(Tensor rowptr, Tensor col, Tensor T, Tensor a_src0, Tensor a_dst0, Tensor u_src, Tensor u_dst, Tensor seg, "
            "Tensor prow, Tensor pptr, int max_rows, Tensor? xrow, Tensor? b0, float slope0, float slope1) -> Tensor")
_LIB.define("sage_graph_query_hops(Tensor rowptr, Tensor col, Tensor val, Tensor T, Tensor seg, Tensor prow, Tensor pptr, int max_rows, "
            "Tensor? xrow, Tensor? b0) -> Tensor")
_LIB.define("gin_graph_query_tail(Tensor G, Tensor pptr, Tensor W1a, Tensor? b1a, Tensor W1b, Tensor? b1b, Tensor Wl, Tensor? bl, int pool, "
            "bool softmax) -> Tensor")


def _spmm_csr(rowptr, col, val, X, tiles, window_rows, bias, epilogue, p, seed, mask):
    return ops.spmm_raw(rowptr, col, val, tiles, X, int(rowptr.numel()) - 1, bias=bias, epilogue=epilogue, p=p, seed=seed,
                        mask=mask, window_rows=window_rows)


def _spmm_csr_pair(rowptr, col, val, tiles, rowptr_t, col_t, val_t, tiles_t, X, window_rows):
    return ops.spmm_raw(rowptr, col, val, tiles, X, int(rowptr.numel()) - 1, window_rows=window_rows)


def _gcn_norm_csr(rowptr, col, w):
    _lib.require_cuda(col)   # col.device places the outputs and names the stream; the call checks the others
    n = int(rowptr.numel()) - 1
    val = torch.empty(col.numel(), dtype=torch.float32, device=col.device)
    dinv = torch.empty(n, dtype=torch.float32, device=col.device)
    _lib.call("fitgnn_gcn_norm_csr_f32", rowptr, col, w, val, dinv, n, _lib.stream_ptr(col.device))
    return val, dinv


def _epilogue_bwd(dOut, out, epilogue, p, seed, mask):
    return ops.epilogue_bwd_raw(dOut, out, epilogue, p=p, seed=seed, mask=mask, want_db=True)


def _pool_rows(assign, cval, n, X):
    return coarsening.pool_rows(assign, cval, n, X)


def _variation_costs(rowptr, col, w, dw, A, set_off, set_mem):
    _lib.require_cuda(rowptr, col, w, dw, A, set_off, set_mem)
    n_sets = int(set_off.numel()) - 1
    K = int(A.shape[1])
    set_len = (set_off[1:] - set_off[:-1]).contiguous()
    cost = torch.empty(n_sets, dtype=torch.float64, device=A.device)
    _lib.call("fitgnn_variation_costs_f64", rowptr, col, w, dw, A, K, int(A.stride(0)), set_off, set_len, set_mem, n_sets, cost,
              _lib.stream_ptr(A.device))
    return cost


def _lift_adjacency(rowptr, col, w, assign, cval, n):
    res = coarsening.LevelResult()
    res.N, res.n, res.assign, res.cval, res.device = int(rowptr.numel()) - 1, int(n), assign, cval, rowptr.device
    res.rowptr, res.col, res.w = rowptr, col, w
    Wc = coarsening.lift_adjacency(res)
    dev = rowptr.device
    return (torch.from_numpy(Wc.indptr.astype("int32")).to(dev), torch.from_numpy(Wc.indices.astype("int32")).to(dev),
            torch.from_numpy(Wc.data).to(dev))


def _gemm_nt(a, b):
    _lib.require_cuda(a, b)
    return ops.gemm_nt(a.contiguous(), b.contiguous())


def _gemm_atb(a, b):
    _lib.require_cuda(a, b)
    return ops.gemm_atb(a.contiguous(), b.contiguous())


def _gcn_query_gather(rowptr, col, val, T, rows, xrow, b0):
    return ops.gcn_query_gather(rowptr, col, val, T, rows, xrow=xrow, b0=b0)


def _gat_query_gather(rowptr, col, T, a_src0, a_dst0, u_src, u_dst, rows, xrow, b0, slope0, slope1):
    return ops.gat_query_gather(rowptr, col, T, a_src0, a_dst0, u_src, u_dst, rows, xrow=xrow, b0=b0, slope0=slope0, slope1=slope1)


def _sage_query_gather(rowptr, col, val, T, rows, xrow, b0):
    return ops.sage_query_gather(rowptr, col, val, T, rows, xrow=xrow, b0=b0)


def _gin_query_hops(rowptr, col, val, T, eps0, W0b, b0b, eps1, rows, xrow, b0a):
    return ops.gin_query_hops(rowptr, col, val, T, eps0, W0b, b0b, eps1, rows, xrow=xrow, b0a=b0a)


def _gin_query_tail(G, W1a, b1a, W1b, b1b, Wl, bl, log_softmax):
    return ops.gin_query_tail(G, W1a, b1a, W1b, b1b, Wl, bl, log_softmax=log_softmax)


def _gcn_query_tail(G, W1, b1, Wl, bl, log_softmax):
    return ops.gcn_query_tail(G, W1, b1, Wl, bl, log_softmax=log_softmax)


def _gcn_graph_query_hops(rowptr, col, val, T, seg, prow, pptr, max_rows, xrow, b0):
    return ops.gcn_graph_query_hops(rowptr, col, val, T, seg, prow, pptr, max_rows, xrow=xrow, b0=b0)


def _gcn_graph_query_tail(G, pptr, W1, b1, Wl, bl, pool, softmax):
    return ops.gcn_graph_query_tail(G, pptr, W1, b1, Wl, bl, pool=("max", "mean")[pool], softmax=softmax)


def _gin_graph_query_hops(rowptr, col, val, T, eps0, W0b, b0b, eps1, seg, prow, pptr, max_rows, xrow, b0a):
    return ops.gin_graph_query_hops(rowptr, col, val, T, eps0, W0b, b0b, eps1, seg, prow, pptr, max_rows, xrow=xrow, b0a=b0a)


def _gin_graph_query_tail(G, pptr, W1a, b1a, W1b, b1b, Wl, bl, pool, softmax):
    return ops.gin_graph_query_tail(G, pptr, W1a, b1a, W1b, b1b, Wl, bl, pool=("max", "mean")[pool], softmax=softmax)


def _gat_graph_query_hops(rowptr, col, T, a_src0, a_dst0, u_src, u_dst, seg, prow, pptr, max_rows, xrow, b0, slope0, slope1):
    return ops.gat_graph_query_hops(rowptr, col, T, a_src0, a_dst0, u_src, u_dst, seg, prow, pptr, max_rows, xrow=xrow, b0=b0, slope0=slope0,
                                    slope1=slope1)


def _sage_graph_query_hops(rowptr, col, val, T, seg, prow, pptr, max_rows, xrow, b0):
    return ops.sage_graph_query_hops(rowptr, col, val, T, seg, prow, pptr, max_rows, xrow=xrow, b0=b0)


for _name, _fn in (("gat_graph_query_hops", _gat_graph_query_hops), ("sage_graph_query_hops", _sage_graph_query_hops), ("gcn_graph_query_hops", _gcn_graph_query_hops), ("gcn_graph_query_tail", _gcn_graph_query_tail),
                   ("gin_graph_query_hops", _gin_graph_query_hops), ("gin_graph_query_tail", _gin_graph_query_tail),
                   ("gcn_query_gather", _gcn_query_gather), ("gat_query_gather", _gat_query_gather), ("sage_query_gather", _sage_query_gather), ("gin_query_hops", _gin_query_hops), ("gin_query_tail", _gin_query_tail), ("gcn_query_tail", _gcn_query_tail), ("gemm_nt", _gemm_nt), ("gemm_atb", _gemm_atb), ("linear", _gemm_nt), ("spmm_csr", _spmm_csr), ("spmm_csr_pair", _spmm_csr_pair), ("gcn_norm_csr", _gcn_norm_csr),
                   ("epilogue_bwd", _epilogue_bwd), ("pool_rows", _pool_rows), ("variation_costs", _variation_costs),
                   ("lift_adjacency", _lift_adjacency)):
    _LIB.impl(_name, _fn, "CUDA")


# ---- fake kernels: shapes / dtypes without touching data (torch.compile tracing, meta tensors) ----
@torch.library.register_fake("fitgnn::spmm_csr")
def _(rowptr, col, val, X, tiles, window_rows, bias, epilogue, p, seed, mask):
    return X.new_empty((rowptr.shape[0] - 1, X.shape[1]))


@torch.library.register_fake("fitgnn::spmm_csr_pair")
def _(rowptr, col, val, tiles, rowptr_t, col_t, val_t, tiles_t, X, window_rows):
    return X.new_empty((rowptr.shape[0] - 1, X.shape[1]))


@torch.library.register_fake("fitgnn::gcn_norm_csr")
def _(rowptr, col, w):
    return col.new_empty(col.shape, dtype=torch.float32), col.new_empty((rowptr.shape[0] - 1,), dtype=torch.float32)


@torch.library.register_fake("fitgnn::epilogue_bwd")
def _(dOut, out, epilogue, p, seed, mask):
    return torch.empty_like(dOut), dOut.new_empty((dOut.shape[1],))


@torch.library.register_fake("fitgnn::pool_rows")
def _(assign, cval, n, X):
    return X.new_empty((n, X.shape[1]), dtype=torch.float32)


@torch.library.register_fake("fitgnn::variation_costs")
def _(rowptr, col, w, dw, A, set_off, set_mem):
    return A.new_empty((set_off.shape[0] - 1,), dtype=torch.float64)


@torch.library.register_fake("fitgnn::gemm_nt")
def _(a, b):
    return a.new_empty((a.shape[0], b.shape[0]))


@torch.library.register_fake("fitgnn::gemm_atb")
def _(a, b):
    return a.new_empty((a.shape[1], b.shape[1]))


@torch.library.register_fake("fitgnn::linear")
def _(x, W):
    return x.new_empty((x.shape[0], W.shape[0]))


@torch.library.register_fake("fitgnn::gcn_query_gather")
def _(rowptr, col, val, T, rows, xrow, b0):
    return T.new_empty((rows.shape[0], T.shape[1]))


@torch.library.register_fake("fitgnn::gat_query_gather")
def _(rowptr, col, T, a_src0, a_dst0, u_src, u_dst, rows, xrow, b0, slope0, slope1):
    return T.new_empty((rows.shape[0], T.shape[1]))


@torch.library.register_fake("fitgnn::sage_query_gather")
def _(rowptr, col, val, T, rows, xrow, b0):
    return T.new_empty((rows.shape[0], T.shape[1]))


@torch.library.register_fake("fitgnn::gin_query_hops")
def _(rowptr, col, val, T, eps0, W0b, b0b, eps1, rows, xrow, b0a):
    return T.new_empty((rows.shape[0], W0b.shape[0]))


@torch.library.register_fake("fitgnn::gin_query_tail")
def _(G, W1a, b1a, W1b, b1b, Wl, bl, log_softmax):
    return G.new_empty((G.shape[0], Wl.shape[0]))


@torch.library.register_fake("fitgnn::gcn_query_tail")
def _(G, W1, b1, Wl, bl, log_softmax):
    return G.new_empty((G.shape[0], Wl.shape[0]))


@torch.library.register_fake("fitgnn::gcn_graph_query_hops")
def _(rowptr, col, val, T, seg, prow, pptr, max_rows, xrow, b0):
    return T.new_empty((prow.shape[0], T.shape[1]))


@torch.library.register_fake("fitgnn::gcn_graph_query_tail")
def _(G, pptr, W1, b1, Wl, bl, pool, softmax):
    return G.new_empty((pptr.shape[0] - 1, Wl.shape[0]))


@torch.library.register_fake("fitgnn::gin_graph_query_hops")
def _(rowptr, col, val, T, eps0, W0b, b0b, eps1, seg, prow, pptr, max_rows, xrow, b0a):
    return T.new_empty((prow.shape[0], W0b.shape[0]))


@torch.library.register_fake("fitgnn::gat_graph_query_hops")
def _(rowptr, col, T, a_src0, a_dst0, u_src, u_dst, seg, prow, pptr, max_rows, xrow, b0, slope0, slope1):
    return T.new_empty((prow.shape[0], T.shape[1]))


@torch.library.register_fake("fitgnn::sage_graph_query_hops")
def _(rowptr, col, val, T, seg, prow, pptr, max_rows, xrow, b0):
    return T.new_empty((prow.shape[0], T.shape[1]))


@torch.library.register_fake("fitgnn::gin_graph_query_tail")
def _(G, pptr, W1a, b1a, W1b, b1b, Wl, bl, pool, softmax):
    return G.new_empty((pptr.shape[0] - 1, Wl.shape[0]))


def _linear_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _linear_backward(ctx, dY):
    x, W = ctx.saved_tensors
    dY = dY.contiguous()
    dX = torch.ops.fitgnn.gemm_nt(dY, W.t().contiguous()) if ctx.needs_input_grad[0] else None
    dW = torch.ops.fitgnn.gemm_atb(dY, x) if ctx.needs_input_grad[1] else None
    return dX, dW


torch.library.register_autograd("fitgnn::linear", _linear_backward, setup_context=_linear_setup)


# ---- autograd: d/dX of Y = A X is A^T dY -- the same kernel on the transposed pattern ----
def _pair_setup(ctx, inputs, output):
    rowptr, col, val, tiles, rowptr_t, col_t, val_t, tiles_t, X, window_rows = inputs
    ctx.save_for_backward(rowptr, col, val, tiles, rowptr_t, col_t, val_t, tiles_t)
    ctx.window_rows = window_rows


def _pair_backward(ctx, dY):
    rowptr, col, val, tiles, rowptr_t, col_t, val_t, tiles_t = ctx.saved_tensors
    dX = torch.ops.fitgnn.spmm_csr_pair(rowptr_t, col_t, val_t, tiles_t, rowptr, col, val, tiles, dY.contiguous(), ctx.window_rows)
    return None, None, None, None, None, None, None, None, dX, None


torch.library.register_autograd("fitgnn::spmm_csr_pair", _pair_backward, setup_context=_pair_setup)


def spmm(g, X):
    """Differentiable Y = A_hat X through torch.ops.fitgnn.spmm_csr_pair for a fitgnn_amd.csr.CSRGraph."""
    f, t = g.f, g.t
    return torch.ops.fitgnn.spmm_csr_pair(f.rowptr, f.col, f.val, f.tiles, t.rowptr, t.col, t.val, t.tiles, X, g.window_rows)
