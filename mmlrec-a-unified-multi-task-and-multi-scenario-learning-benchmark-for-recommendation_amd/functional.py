"""Stand-alone differentiable wrappers over single C-ABI ops, for code that calls a parameter container directly
(e.g. `DNN.forward`) instead of going through a model's step plan."""
import torch

from . import _lib as L
from . import ops


class _LinearAct(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, W, b, act):
        x = x.contiguous()
        out = torch.empty(x.shape[0], W.shape[0], dtype=torch.float32, device=x.device)
        ops.gemm_fwd([dict(A=x, W=W, bias=b, C=out, act=act)])
        ctx.save_for_backward(x, W, out)
        ctx.act, ctx.has_b = act, b is not None
        return out

    @staticmethod
    def backward(ctx, dy):
        x, W, out = ctx.saved_tensors
        dz = torch.empty_like(out)
        ops.act_bwd(out, dy.contiguous(), dz, ctx.act)
        dx = torch.empty_like(x)
        ops.gemm_dgrad([dict(dA=dx, Y=None, srcs=[(dz, W, 0)])])
        dW = torch.empty_like(W)
        db = torch.empty(W.shape[0], device=W.device) if ctx.has_b else None
        ops.gemm_wgrad([dict(dC=dz, A=x, dW=dW, dbias=db)])
        return dx, dW, db, None


def linear_act(x, W, b=None, act=L.ACT_NONE):
    """act(x @ W^T + b) on the fp32 MFMA GEMM kernels (K3), differentiable."""
    if not x.is_cuda:
        raise L.MMLError("mmlrec_amd.functional needs CUDA(HIP) tensors; there is no CPU fallback")
    return _LinearAct.apply(x.float(), W, b, int(act))


class _PReLU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, alpha):
        y = torch.empty_like(z)
        ops.prelu_fwd([dict(z=z, y=y, alpha=alpha)])
        ctx.save_for_backward(z, alpha)  # (z, not y: for alpha <= 0 the sign of y does not give the sign of z)
        return y

    @staticmethod
    def backward(ctx, dy):
        z, alpha = ctx.saved_tensors
        dz, da = torch.empty_like(z), torch.empty_like(alpha)
        ops.prelu_bwd([dict(dy=dy.contiguous(), z=z, dz=dz, alpha=alpha, dalpha=da)])
        return dz, da


def prelu(z, alpha):
    """PReLU with ONE slope (nn.PReLU()'s weight, a one-element tensor): z > 0 ? z : alpha * z on a [B, n] value,
    differentiable in both (K: mml_prelu_batch_fwd / _bwd; torch.nn.functional.prelu's semantics)."""
    if not z.is_cuda:
        raise L.MMLError("mmlrec_amd.functional needs CUDA(HIP) tensors; there is no CPU fallback")
    if z.dim() != 2 or alpha.numel() != 1:
        raise L.MMLError("functional.prelu: a [B, n] value and a one-element slope")
    return _PReLU.apply(z.float().contiguous(), alpha)


class _PooledDnnInput(torch.autograd.Function):
    @staticmethod
    def forward(ctx, X, layout, status, *tables):
        pooled = [ops.PooledField(c0, T, comb, tb, lc) for c0, T, comb, tb, lc in layout["pooled"]]
        out, argmax, _ = ops.gather_pool_fwd([t.detach() for t in tables], X, layout["singles"], pooled,
                                             layout["dense_col0"], layout["nd"], status=status)
        ctx.save_for_backward(X, argmax)
        ctx.layout, ctx.pooled, ctx.status = layout, pooled, status
        ctx.table_meta = [(t.shape, t.dtype, t.device, t.requires_grad) for t in tables]  # (the rows are not needed again)
        return out

    @staticmethod
    def backward(ctx, d_out):
        X, argmax = ctx.saved_tensors
        grads = [torch.zeros(sh, dtype=dt, device=dv) for sh, dt, dv, _ in ctx.table_meta]
        n_emb = (len(ctx.layout["singles"]) + len(ctx.pooled)) * grads[0].shape[1]  # (the dense columns are input data)
        ops.scatter_pool_bwd(grads, X, ctx.layout["singles"], ctx.pooled, d_out[:, :n_emb].contiguous(), argmax=argmax,
                             status=ctx.status)
        return (None, None, None) + tuple(g if m[3] else None for g, m in zip(grads, ctx.table_meta))


def pooled_dnn_input(embedding_dict, X, layout, status=None):
    """dnn_input of a schema with multi-valued (VarLenSparseFeat) columns, differentiable in the tables.

    embedding_dict: {embedding name: nn.Embedding} (model.utils.create_embedding_matrix), layout:
    model.utils.pooled_layout(feature_columns), X: the fp32 [B, columns] input matrix.  ONE gather launch forward
    (mml_gather_pool_fwd), ONE scatter launch backward (mml_scatter_pool_bwd: dense [V, E] gradients like
    nn.Embedding(sparse=False), a shared table accumulating over its fields).
    status: an ops.new_status(device) word the launches raise for an out-of-range id at a VALID position; the caller
    turns it into nn.Embedding's IndexError with ops.check_status(status) whenever it can afford the synchronisation
    (once per epoch, say) -- no call here synchronises.  Such an id is clamped into the table, never used as it is."""
    if not X.is_cuda:
        raise L.MMLError("mmlrec_amd.functional needs CUDA(HIP) tensors; there is no CPU fallback")
    tables = [embedding_dict[n].weight for n in layout["table_names"]]
    return _PooledDnnInput.apply(X.float().contiguous(), layout, status, *tables)
