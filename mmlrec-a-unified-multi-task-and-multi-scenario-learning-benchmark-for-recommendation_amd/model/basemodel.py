"""BaseModel: the nn.Module contract of the reference (model/basemodel.py:69-650) -- constructor validation,
`forward(X, domain_mask)`, `compile / fit / evaluate / predict`, state_dict keys -- on top of static HIP step plans.

What differs from the reference by design:
  * forward() never runs ATen math: it replays a recorded list of C-ABI kernel launches (engine.Plan).
  * fit() keeps X / y resident on the GPU, runs ONE fused step (fwd + summed BCE + bwd + optimizer, optionally as a
    HIP graph) per batch, and computes the sklearn metrics once per epoch off the hot path instead of per step
    (reference :316-331) -- the numbers printed per epoch are the same quantities.
  * reference defects D2/D3/D7 are handled as documented there: the domain mask is None inside
    fit/predict exactly like the reference's tautological condition makes it, predict() derives the mask only from
    mapping inputs, and fit() returns self when no validation epoch improved.
There is no CPU execution path: tensors must live on an MI355X.
"""
import copy
import time

import numpy as np
import torch
import torch.nn as nn

from .. import _lib as L
from .. import bind
from .. import engine as E
from .. import optimizer as O
from .. import ops
from .. import profiling
from .utils import (DenseFeat, PredictionLayer, SparseFeat, VarLenSparseFeat, build_input_features,
                    create_embedding_matrix)


class Linear(nn.Module):
    """Wide part of the reference (model/basemodel.py:14-66).  Every hot-path model passes no linear columns, so it
    owns no parameters; kept so module trees / state_dict layouts line up."""

    def __init__(self, feature_columns, feature_index, init_std=0.0001, device="cpu"):
        super().__init__()
        if len(feature_columns):
            raise NotImplementedError("linear (wide) feature columns are outside the MI355X hot path")
        self.feature_index = feature_index
        self.embedding_dict = nn.ModuleDict()


class _PlanFunction(torch.autograd.Function):
    """Makes one recorded plan look like a differentiable op: forward replays the forward launches, backward feeds
    dL/dprob into the head kernel and replays the backward launches; gradients come back per parameter (tables as
    dense [V,E] tensors, like the reference's sparse=False embeddings)."""

    @staticmethod
    def forward(ctx, model, plan, X, mask, *params):
        model._load_batch(plan, X, mask)
        plan.run_forward()
        ctx.model, ctx.plan = model, plan
        plan.generation += 1
        ctx.generation = plan.generation
        return plan.prob.clone()

    @staticmethod
    def backward(ctx, dprob):
        plan, model = ctx.plan, ctx.model
        if ctx.generation != plan.generation:
            raise RuntimeError("mmlrec_amd: backward() of a forward whose plan buffers were overwritten by a later "
                               "forward of the same batch size; call backward before the next forward")
        plan.dprob.copy_(dprob)
        plan.run_backward_from_dprob()
        store = model._store()
        grads = []
        for name, p in model.named_parameters():
            pv = store.pvals[name]
            # (the set THIS plan's backward writes, taken when it was recorded: the store's `written` counters belong
            # to whichever plan was recorded last -- a no_grad forward of a new batch size between this forward and its
            # backward resets them)
            if name not in plan.written_names or pv.grad is None:
                grads.append(None)
            elif pv.is_table:
                grads.append(pv.grad.clone())
                pv.grad.zero_()
            else:
                grads.append(pv.grad.clone())
        return (None, None, None, None) + tuple(grads)


class BaseModel(nn.Module):
    num_outputs = None      # columns of forward()'s result when that differs from num_tasks (ESCM: 3 for 2 tasks)
    metric_columns = None   # ... and the output columns the metrics are computed on (basemodel.py:326-327)
    binary_only = None      # models whose outputs are products of probabilities or constraints on them: the reason they
                            # refuse regression tasks and losses other than binary_crossentropy (ESMM, ESCM, AITM)
    LOSS_KINDS = {"binary_crossentropy": L.HEAD_LOSS_BCE, "mse": L.HEAD_LOSS_MSE, "mae": L.HEAD_LOSS_MAE}
    METRIC_KINDS = {"auc": "binary", "acc": "binary", "accuracy": "binary", "logloss": "binary",
                    "binary_crossentropy": "binary", "mse": "regression"}

    def __init__(self, linear_feature_columns, dnn_feature_columns, init_std=0.0001, device="cpu", gpus=None,
                 config=None):
        super().__init__()
        self.dnn_feature_columns = dnn_feature_columns
        self.config = config
        self.data_config = config["data_config"]
        self.model_config = config["model_config"]
        self.optim_config = config["optim_config"]
        self.training_config = config["training_config"]
        self.save_layer_output = False
        self.use_cka_loss = self.model_config.get("use_cka_loss", False)
        if self.use_cka_loss:
            raise NotImplementedError("use_cka_loss: the reference imports a module that does not exist (SURVEY D14)")
        self.device = device
        self.gpus = gpus
        # key of the dropout mask stream (engine.DropoutOp): the seed torch's global generator was given, so that a
        # seeded run (main.set_seed) repeats; the masks themselves are not torch's (include/mmlrec.h: mml_dropout)
        self.dropout_seed = int(torch.initial_seed()) & ((1 << 64) - 1)
        if gpus and str(self.gpus[0]) not in str(self.device):
            raise ValueError("`gpus[0]` should be the same gpu with `device`")

        self.task_name = self.model_config.get("task_name", "mtl")
        self.task_names = self.model_config.get("task_names", ["ctr", "ctcvr"])
        self.task_types = self.model_config.get("task_types", ["binary", "binary"])
        self.num_domains = self.data_config.get("num_domains", 1)
        if self.task_name == "msl":
            self.num_tasks = self.num_domains
        elif self.task_name == "mtmsl":
            self.num_tasks = len(self.data_config["label_columns"])
        else:
            self.num_tasks = len(self.task_names)
        if self.num_tasks <= 1:
            raise ValueError("num_tasks must be greater than 1!")
        if len(dnn_feature_columns) == 0:
            raise ValueError("dnn_feature_columns is null!")
        if len(self.task_types) != self.num_tasks:
            raise ValueError("num_tasks must be equal to the length of task_types")
        for task_type in self.task_types:
            if task_type not in ["binary", "regression"]:
                raise ValueError("task must be binary or regression, {} is illegal".format(task_type))
            if task_type != "binary" and self.binary_only:
                raise NotImplementedError(f"{type(self).__name__}: task type {task_type!r}: {self.binary_only}")
        if any(isinstance(f, VarLenSparseFeat) for f in dnn_feature_columns):
            from .utils import pooled_layout
            pooled_layout(dnn_feature_columns)  # (one embedding_dim, known combiners, equal sizes of a shared table)
            if any(isinstance(f, VarLenSparseFeat) for f in linear_feature_columns):
                raise NotImplementedError("VarLenSparseFeat in the wide (linear) columns")
        l2_reg_linear = self.model_config.get("l2_reg_linear", 1e-5)
        l2_reg_embedding = self.model_config.get("l2_reg_embedding", 1e-5)

        self.feature_index = build_input_features(list(linear_feature_columns) + list(dnn_feature_columns))
        self.embedding_dict = create_embedding_matrix(dnn_feature_columns, init_std, sparse=False, device=device)
        self.linear_model = Linear(linear_feature_columns, self.feature_index, device=device)
        self.regularization_weight = []
        self.add_regularization_weight(self.embedding_dict.parameters(), l2=l2_reg_embedding)
        self.add_regularization_weight(self.linear_model.parameters(), l2=l2_reg_linear)
        self.out = PredictionLayer(self.model_config.get("task", "binary"))
        self._caches = {"store": None, "plans": {}, "steps": {}}
        self.table_update = self.model_config.get("table_update", "auto")  # additive key: auto|dense_exact|sparse_rows
        self.use_hip_graph = bool(self.model_config.get("use_hip_graph", True))
        # additive key, off by default: whole-set and large-batch metrics on the device
        self.device_metrics = self._parse_switch(self.optim_config.get("device_metrics", False))
        self.to(device)

    # ---- schema helpers ------------------------------------------------------------------------
    def _sparse_cols(self):
        return [f for f in self.dnn_feature_columns if isinstance(f, SparseFeat)]

    def _pooled_cols(self):
        return [f for f in self.dnn_feature_columns if isinstance(f, VarLenSparseFeat)]

    def _lookups_per_sample(self):
        """Table rows one sample can name: the bound of the touched-row list per sample."""
        return len(self._sparse_cols()) + sum(int(f.maxlen) for f in self._pooled_cols())

    def _refuse_pooled_before(self, scene_feature):
        """PepNet / APG take the scene embedding as sparse_embedding_list[feature_index[scene][0]] (reference
        model/pepnet.py:97,126): the scene's X COLUMN used as a LIST position.  A pooled feature declared in front of it
        shifts the column by maxlen and the list position by nothing, so the reference reads another feature's block."""
        for f in self.dnn_feature_columns:
            if f.name == scene_feature:
                return
            if isinstance(f, VarLenSparseFeat):
                raise NotImplementedError(
                    f"{type(self).__name__}: the pooled feature {f.name!r} is declared before the scene feature "
                    f"{scene_feature!r}; declare multi-valued features after all single-valued ones")

    def _dense_cols(self):
        return [f for f in self.dnn_feature_columns if isinstance(f, DenseFeat)]

    def compute_input_dim(self, feature_columns, include_sparse=True, include_dense=True, feature_group=False):
        sp = [f for f in feature_columns if isinstance(f, (SparseFeat, VarLenSparseFeat))]
        de = [f for f in feature_columns if isinstance(f, DenseFeat)]
        dim = 0
        if include_sparse:
            dim += len(sp) if feature_group else sum(f.embedding_dim for f in sp)
        if include_dense:
            dim += sum(f.dimension for f in de)
        return dim

    @property
    def embedding_size(self):
        sizes = {f.embedding_dim for f in self._sparse_cols() + self._pooled_cols()}
        if len(sizes) > 1:
            raise ValueError("embedding_dim of SparseFeat and VarlenSparseFeat must be same in this model!")
        return list(sizes)[0]

    # ---- regularisation API (reference :510-540) -------------------------------------------------
    def add_regularization_weight(self, weight_list, l1=0.0, l2=0.0):
        weight_list = [weight_list] if isinstance(weight_list, nn.Parameter) else list(weight_list)
        self.regularization_weight.append((weight_list, l1, l2))

    def _has_regularization(self):
        return any((l1 > 0 or l2 > 0) and len(w) for w, l1, l2 in self.regularization_weight)

    def get_regularization_loss(self):
        total = torch.zeros((1,), device=self.device)
        for weight_list, l1, l2 in self.regularization_weight:
            for w in weight_list:
                p = w[1] if isinstance(w, tuple) else w
                if l1 > 0:
                    total = total + torch.sum(l1 * torch.abs(p))
                if l2 > 0:
                    total = total + torch.sum(l2 * torch.square(p))
        return total

    def update_save(self, value=True):
        self.save_layer_output = value

    # ---- plan management -------------------------------------------------------------------------
    def __deepcopy__(self, memo):
        self.flush_tables()
        caches = self._caches
        self.__dict__["_caches"] = {"store": None, "plans": {}, "steps": {}}
        try:
            cls = self.__class__
            new = cls.__new__(cls)
            memo[id(self)] = new
            for k, v in self.__dict__.items():
                # the fused optimizer (moments, gradient accumulators) stays with the live model: the copy is the
                # "best model" snapshot used for predict(), like the reference's deepcopy(model) (basemodel.py:344)
                new.__dict__[k] = None if k == "_optimizer" else copy.deepcopy(v, memo)
        finally:
            self.__dict__["_caches"] = caches
        return new

    def _apply(self, fn, *a, **k):
        if "_caches" in self.__dict__ and getattr(self, "_optimizer", None) is not None:
            self.flush_tables()  # (model.to() / .float(): the store and its optimizer are rebuilt on the new storage)
        out = super()._apply(fn, *a, **k)
        if "_caches" in self.__dict__:
            self._caches = {"store": None, "plans": {}, "steps": {}}
        try:
            self.device = next(self.parameters()).device
        except StopIteration:
            pass
        return out

    def _store(self):
        st = self._caches["store"]
        if st is None or st.stale():
            old = getattr(self, "_optimizer", None)
            if (st is not None and old is not None and old.store is st and old.table_update == "lazy_exact" and
                    old.dirty and old.last is not None):
                # the parameters were re-seated behind the optimizer's back (p.data = ...): the pending replays of the
                # old storage cannot be applied to the new one
                raise L.MMLError("parameter storage replaced while lazy_exact table updates were pending: call "
                                 "model.flush_tables() before re-seating parameters")
            dev = next(self.parameters()).device
            if dev.type != "cuda":
                raise L.MMLError("mmlrec_amd models run on an MI355X only: move the model to cuda (no CPU fallback)")
            st = O.ParamStore(self, dev)
            self._caches = {"store": st, "plans": {}, "steps": {}}
        return st

    def _get_plan(self, B, training, masked):
        store = self._store()
        # (BatchNorm follows the MODULE's mode, whether or not gradients are recorded: it is part of the key)
        key = (int(B), bool(training), bool(masked), bool(self.training))
        plan = self._caches["plans"].get(key)
        if plan is None:
            plan = self._record(B, training, masked, store)
            self._caches["plans"][key] = plan
        return plan

    def _record(self, B, training, masked, store, sparse_rows=None, lazy=False, mark_rows=None, grad_marks=False,
                pcgrad=False):
        plan = E.Plan(store.device, B, training, use_amax=False if pcgrad else None)
        plan.bn_training = bool(self.training)
        plan.dropout_on = bool(self.training)
        plan.dropout_seed = int(getattr(self, "dropout_seed", 0))
        par0 = getattr(self, "_parallel", None)
        # data-parallel ranks hold consecutive blocks of the global batch (rank r: rows [r B, (r + 1) B)) and must have
        # been built under the same torch seed: together they then draw the dropout mask of a one-rank step
        plan.row0 = par0.rank * int(B) if (par0 is not None and training) else 0
        if getattr(self, "optim_name", None) is not None:
            plan.step_dev = self.optimizer().step_dev
        else:
            # an uncompiled model: ONE counter for all its plans (every training-mode forward bumps it, see below) and a
            # step word per PLAN that holds the value its latest forward drew -- the backward regenerates the mask from the
            # plan's word, so a forward of another plan (another batch size, the masked variant, a no_grad forward) between
            # a forward and its backward cannot change it
            own = self.__dict__.get("_own_step_dev")
            if own is None or own.device != store.device:
                own = self.__dict__["_own_step_dev"] = torch.zeros(1, dtype=torch.int32, device=store.device)
            plan.shared_step_dev = own
            plan.step_dev = plan.zeros(1, dtype=torch.int32)
        plan.generation = 0
        sp, de = self._sparse_cols(), self._dense_cols()
        ftot = max(e for _, e in self.feature_index.values())
        plan.X = plan.zeros(B, ftot)
        T = self.num_tasks
        if training:
            plan.y = plan.zeros(B, T)
            store.ensure_table_grads()
        if masked:
            plan.mask = plan.zeros(B, max(self.num_domains, 1))
        if pcgrad:
            # PCGrad per-task step: head t reads column t of a per-head mask the schedule rewrites before every
            # objective's pass (1 in that objective's column, 0 elsewhere: a zero seed for the other heads)
            if masked or not training:
                raise L.MMLError("a PCGrad per-task plan is an unmasked training plan")
            plan.pcgrad_T = T
            plan.mask = plan.zeros(B, T)
        store.reset_written()
        E_dim = self.embedding_size
        nd = sum(f.dimension for f in de)
        dense_col0 = self.feature_index[de[0].name][0] if de else 0
        if de:  # the gather copies ONE contiguous run of dense columns (ctrdataset lays them out that way)
            pos = dense_col0
            for f in de:
                if self.feature_index[f.name][0] != pos:
                    raise NotImplementedError("dense feature columns must be contiguous in X")
                pos += f.dimension
        par_ = getattr(self, "_parallel", None)
        vl = self._pooled_cols()
        if vl:
            if par_ is not None:
                raise NotImplementedError("multi-valued (pooled) features on sharded / replicated tables")
            # The deterministic pooled scatter (mml_scatter_pool_bwd_det) is asked for by name: scatter_mode alone keeps
            # the refusal it has had since pooled features came, which callers and the suite rely on.
            if self._scatter_mode() == "deterministic" and training and not self._pooled_deterministic():
                raise NotImplementedError("scatter_mode='deterministic' with multi-valued (pooled) features: set "
                                          "model.pooled_deterministic = True (or model_config['pooled_deterministic']) "
                                          "to sum their table gradients with the deterministic pooled scatter")
            if mark_rows is not None:
                raise NotImplementedError("the row-marking gather of the split dense update has no pooled form")
        # (pooled fields: dnn_input stays fp32 -- the pooled gather has no bf16-storage form)
        x0 = plan.val((len(sp) + len(vl)) * E_dim + nd, needs_grad=training, name="dnn_input", pad_k=True,
                      store16=(plan.bf16 and par_ is None and mark_rows is None and E_dim % 4 == 0 and not vl and
                               self._dnn_input_store16(plan)))
        if nd:
            x0.grad_cols = (len(sp) + len(vl)) * E_dim  # the dense features' gradient has no reader (they are input data)
        if vl:
            from .utils import pooled_layout
            lay = pooled_layout(self.dnn_feature_columns, self.feature_index)
            ptabs = [store.pvals[f"embedding_dict.{n}.weight"] for n in lay["table_names"]]
            if [f"embedding_dict.{n}.weight" for n in lay["table_names"]] != list(store.table_names):
                raise L.MMLError("pooled gather: the tables of the layout are not the store's tables")
            gop = E.PooledGatherOp(ptabs, plan.X, lay["singles"], lay["pooled"], dense_col0, nd, x0,
                                   sparse_rows=sparse_rows)
            if grad_marks and training and sparse_rows is None:
                gop.grad_marks = store.ensure_grad_marks(ptabs)[0]
            # (the op names every table once: fields may share a table, their totals are per table)
            self._maybe_deterministic(gop, store, ptabs, training, E_dim)
            plan.add(gop)
            plan.layer_outputs["dnn_input"] = x0
            return self._finish_record(plan, store, x0)
        tables = [store.pvals[f"embedding_dict.{f.embedding_name}.weight"] for f in sp]
        cols = [self.feature_index[f.name][0] for f in sp]
        par = getattr(self, "_parallel", None)
        if par is not None and training and par.mode in ("table_wise", "row_sharded"):
            # the owner-side scatter of these modes is the float-atomic kernel: a deterministic request must not be
            # dropped silently
            self._reject_deterministic(par.mode)
        if par is not None and par.mode == "table_wise":
            from ..parallel import ShardedGatherOp
            plan.add(ShardedGatherOp(par, tables, plan.X, cols, dense_col0, nd, x0, sparse_rows=sparse_rows))
        elif par is not None and training and par.mode == "row_sharded":
            from ..parallel import RowShardedGatherOp
            op = RowShardedGatherOp(par, store.pvals["embedding_shard"], plan.X, cols, dense_col0, nd, x0,
                                    sparse_rows=sparse_rows)
            if grad_marks and sparse_rows is None and E_dim in (4, 8, 16):
                op.grad_marks = store.ensure_grad_marks(op.tables)[0]
            plan.add(op)
        elif par is not None and training and par.mode == "replicated":
            from ..parallel import ReplicatedGatherOp
            op = ReplicatedGatherOp(par, tables, plan.X, cols, dense_col0, nd, x0, sparse_rows=sparse_rows)
            op.x_in_pre = bool(lazy)  # lazy_exact gathers the global index matrix before its catch-up pass
            if (grad_marks and sparse_rows is None and E_dim in (4, 8, 16) and
                    len({id(t) for t in tables}) == len(tables)):
                op.grad_marks = store.ensure_grad_marks(tables)[0]
            self._maybe_deterministic(op, store, tables, training, E_dim)
            plan.add(op)
        else:  # single GPU, and inference on the (synchronised) full tables of a row-sharded / replicated model
            gop = E.GatherOp(tables, plan.X, cols, dense_col0, nd, x0, sparse_rows=sparse_rows)
            gop.mark_rows = mark_rows
            # marked-gradient dense table update (trainer.TrainStep decides): needs the LDS-fold scatter (E in 4, 8, 16)
            # and one table per field (a table shared by two fields would be marked in two maps)
            if (grad_marks and training and sparse_rows is None and E_dim in (4, 8, 16) and
                    len({id(t) for t in tables}) == len(tables)):
                gop.grad_marks = store.ensure_grad_marks(tables)[0]
            self._maybe_deterministic(gop, store, tables, training, E_dim)
            plan.add(gop)
        plan.layer_outputs["dnn_input"] = x0
        return self._finish_record(plan, store, x0)

    def _finish_record(self, plan, store, x0):
        head = self._build_graph(plan, store, x0)
        head.mask_cols = list(range(self.num_tasks)) if plan.pcgrad_T else self._head_mask_cols()
        if plan.pcgrad_T and len(head.heads) != self.num_tasks:
            raise NotImplementedError("PCGrad per_task: one head per task")
        if len(head.heads) == self.num_tasks:  # head t is task t's PredictionLayer
            for t, h in enumerate(head.heads):
                h.setdefault("kind", self._head_kind(t))
        elif any(t != "binary" for t in self.task_types) and any("kind" not in h for h in head.heads):
            raise NotImplementedError(f"{type(self).__name__}: {len(head.heads)} heads for {self.num_tasks} tasks with a "
                                      "regression task: the model must name each head's kind itself")
        plan.finish(head)
        plan.written_names = {n for n, pv in store.pvals.items() if pv.written}
        if (getattr(self, "optim_name", None) is None and plan.dropout_on and
                any(isinstance(o, E.DropoutOp) for o in plan.ops)):
            # an uncompiled model in a custom training loop: the plan owns its step counter, and nothing else would ever
            # move it -- every forward would draw the SAME dropout mask.  The forward bumps it first; the
            # backward of that forward regenerates the mask from the same value.
            own = plan.shared_step_dev
            plan.prepend([plan.bound(bind.counter_update(own, 1, False), kernel="mml_counter_update", bytes=4.0),
                          # (a 4-byte copy: the kernel moves the word's bits unchanged)
                          plan.bound(bind.copy_flat(own, plan.step_dev, False), kernel="copy2d_kernel", bytes=8.0)])
        return plan

    def _maybe_deterministic(self, gop, store, tables, training, E_dim):
        """model.scatter_mode = "deterministic" (or model_config["scatter_mode"]): the table gradients of the step are
        summed in order-independent integer fixed point (mml_scatter_bwd_det; mml_scatter_pool_bwd_det with multi-valued
        features) -- bitwise repeatable runs, and replicated tables that stay bitwise equal on every rank without
        re-broadcasts.  Default "atomic" (float atomics: faster)."""
        mode = self._scatter_mode()
        if mode == "deterministic" and training:
            if E_dim not in (4, 8, 16) or len({id(t) for t in tables}) != len(tables):
                raise NotImplementedError("deterministic scatter: embedding size 4, 8 or 16 and one table per field")
            gop.deterministic = store.ensure_det(tables)

    def _scatter_mode(self):
        mode = getattr(self, "scatter_mode", None) or (self.config or {}).get("model_config", {}).get("scatter_mode", "atomic")
        if mode not in ("atomic", "deterministic"):
            raise ValueError("scatter_mode must be 'atomic' or 'deterministic'")
        return mode

    def _pooled_deterministic(self):
        """model.pooled_deterministic (or model_config["pooled_deterministic"]): with scatter_mode = "deterministic", a
        model with multi-valued (pooled) features sums their table gradients with mml_scatter_pool_bwd_det too.  Default
        off: scatter_mode alone refuses such a model, as it always has."""
        own = getattr(self, "pooled_deterministic", None)
        if own is None:
            own = (self.config or {}).get("model_config", {}).get("pooled_deterministic", False)
        return bool(own)

    def _reject_deterministic(self, where):
        if self._scatter_mode() == "deterministic":
            raise NotImplementedError(
                f"scatter_mode='deterministic' is not available with {where} tables (their owner-side scatter sums with "
                "float atomics); use mode='replicated' or a single GPU for bitwise-repeatable table gradients")

    def _head_mask_cols(self):
        """Column of domain_mask that multiplies head i (e.g. model/mmoe.py:101-106), or None for unmasked heads."""
        if self.task_name in ("msl", "mtmsl"):
            return [i if self.task_name == "msl" else i % self.num_domains for i in range(self.num_tasks)]
        return None

    def _head_kind(self, t):
        """mml_head_desc.kind of head t (include/mmlrec.h, K5): PredictionLayer(task_types[t])'s output form, and the loss
        compile() named for the task -- before compile (forward, autograd through dprob) only the output form is read."""
        out = L.HEAD_OUT_IDENTITY if self.task_types[t] == "regression" else L.HEAD_OUT_SIGMOID
        names = getattr(self, "loss_func", None)
        if names is None:
            loss = L.HEAD_LOSS_MSE if out == L.HEAD_OUT_IDENTITY else L.HEAD_LOSS_BCE
        else:
            loss = self.LOSS_KINDS[names[t]]
        return L.head_kind(out, loss)

    def _build_graph(self, plan, store, x0):
        raise NotImplementedError

    def _dnn_input_store16(self, plan):
        """bf16-storage path (engine.Plan.bf16): True when ONLY bf16-storage layer groups read dnn_input in this model's
        graph, so that the gather may write it as bf16 (models override; Plan.finish checks the promise)."""
        return False

    def flush_tables(self):
        """lazy_exact table optimizer: replay the zero-gradient steps of rows the recent batches did not touch, so that
        every table equals what the reference's dense optimizer holds.  Called automatically by forward / predict /
        state_dict / deepcopy; a no-op for the other table-update modes."""
        opt = getattr(self, "_optimizer", None)
        if opt is not None:
            opt.flush()
        par = getattr(self, "_parallel", None)
        if par is not None and par.dirty:  # collective: every rank reaches this point (parallel.py)
            from ..parallel import sync_tables
            sync_tables(self)

    def state_dict(self, *args, **kwargs):
        self.flush_tables()
        return super().state_dict(*args, **kwargs)

    def _load_batch(self, plan, X, mask=None, y=None):
        if X.shape != plan.X.shape:
            raise L.MMLError(f"X has shape {tuple(X.shape)}, the model expects [B, {plan.X.shape[1]}]")
        plan.X.copy_(X)
        if mask is not None:
            plan.mask.copy_(mask)
        if y is not None:
            plan.y.copy_(y.reshape(plan.y.shape))

    # ---- nn.Module contract ----------------------------------------------------------------------
    def forward(self, X, domain_mask=None):
        """model(X [B,Ftot] float32 with indices stored as floats, domain_mask [B,D] or None) -> probabilities [B,T]
        (reference e.g. model/mmoe.py:65-119)."""
        if not isinstance(X, torch.Tensor) or not X.is_cuda:
            raise L.MMLError("mmlrec_amd: forward() needs a CUDA(HIP) tensor on an MI355X; there is no CPU fallback")
        X = X.float()
        self.flush_tables()
        masked = domain_mask is not None and self.task_name in ("msl", "mtmsl")
        if masked:
            domain_mask = domain_mask.float()
        need_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        plan = self._get_plan(X.shape[0], need_grad, masked)
        if need_grad:
            out = _PlanFunction.apply(self, plan, X, domain_mask if masked else None, *list(self.parameters()))
        else:
            self._load_batch(plan, X, domain_mask if masked else None)
            plan.run_forward()
            out = plan.prob.clone()
        if not getattr(self, "_defer_status", False):  # predict() checks once after its last batch (one host sync)
            ops.check_status(plan.status, "embedding lookup (nn.Embedding semantics)")
        if not self.training and self.save_layer_output:
            self.layer_output_dict = self._collect_layer_outputs(plan)
        return out

    def _collect_layer_outputs(self, plan):
        out = {}
        for k, v in plan.layer_outputs.items():
            if isinstance(v, (list, tuple)):
                out[k] = torch.stack([getattr(x, "buf", x).float() for x in v], 1).clone()
            else:
                out[k] = getattr(v, "buf", v).float().clone()  # (bf16-storage plans keep some values as bf16)
        return out

    # ---- compile (reference :557-647) ------------------------------------------------------------
    @staticmethod
    def _parse_switch(v):
        """A boolean switch as a config file may spell it (true / false, 1 / 0, "true" / "off" ...)."""
        if isinstance(v, str):
            if v.strip().lower() in ("1", "true", "yes", "y", "on"):
                return True
            if v.strip().lower() in ("", "0", "false", "no", "n", "off", "none"):
                return False
            raise ValueError(f"device_metrics: expected a boolean, got {v!r}")
        return bool(v)

    def compile(self, optimizer, loss=None, metrics=None, device_metrics=None):
        """device_metrics: True / False sets the model's `device_metrics` switch (evaluate and the per-batch metrics of
        batches above 4096 rows on the device); None leaves it as optim_config["device_metrics"] or the attribute set it."""
        if device_metrics is not None:
            self.device_metrics = self._parse_switch(device_metrics)
        # a second compile (new optimizer / lr for a second training phase) drops the fused optimizer: rows whose
        # zero-gradient steps are still pending under lazy_exact must replay them first, or the tables silently leave
        # the reference's dense trajectory
        self.flush_tables()
        self.metrics_names = ["loss"]
        if isinstance(optimizer, str):
            if optimizer not in ("sgd", "adam", "adagrad", "rmsprop"):
                raise NotImplementedError
            self.optim_name = optimizer
        else:
            raise NotImplementedError("pass the optimizer by name: the update runs in the fused HIP optimizer kernels")
        if self._pcgrad_objectives() == "per_task":
            # the reference's class has no place for the regulariser among per-task objectives (it is part of neither
            # list entry): no rule is invented here
            mc = self.model_config
            if (any(float(mc.get(k, 0) or 0) != 0 for k in ("l2_reg_embedding", "l2_reg_dnn", "l2_reg_linear")) or
                    any(l1 > 0 or l2 > 0 for _, l1, l2 in getattr(self, "regularization_weight", []))):
                raise ValueError("pcgrad_objectives='per_task' with a regulariser (l2_reg_embedding / l2_reg_dnn / "
                                 "l2_reg_linear): PCGrad has no rule for it among per-task objectives; set them to 0")
        self.loss_func = self._get_loss_func(loss)
        self.metrics = self._get_metrics(metrics)
        self._caches["steps"] = {}
        self._optimizer = None

    def _pcgrad_objectives(self):
        """optim_config["pcgrad_objectives"] of a `pcg` model (reference model/optimizer.py:10-138, model/basemodel.py:309-310,
        :564-565): "total" (default) -- the reference's literal behaviour, pc_backward(total_loss) iterates a one-element
        tensor, ONE objective, no projection can fire: the MMoE step -- or "per_task" -- the list of per-task loss terms
        the class's docstring asks for (trainer.PCGradSchedule).  None for every other model, where a non-default value is
        an error."""
        v = (getattr(self, "optim_config", None) or {}).get("pcgrad_objectives", "total")
        if v not in ("total", "per_task"):
            raise ValueError("optim_config['pcgrad_objectives'] must be 'total' or 'per_task'")
        if self.model_config.get("model_name") != "pcg":
            if v != "total":
                raise ValueError("optim_config['pcgrad_objectives'] is read for model_name 'pcg' only")
            return None
        return v

    def _get_loss_func(self, loss):
        """One loss name per task (reference :586-603): binary_crossentropy, mse (F.mse_loss) or mae (F.l1_loss), each summed
        over the batch; the head kernels evaluate them (include/mmlrec.h, K5: MML_HEAD_LOSS_*)."""
        names = list(loss) if isinstance(loss, (list, tuple)) else [loss] * self.num_tasks
        if len(names) != self.num_tasks:
            raise ValueError("the length of `loss` should be equal with `self.num_tasks`")
        for n, task_type in zip(names, self.task_types):
            if n not in self.LOSS_KINDS:
                raise NotImplementedError(f"loss {n!r}: the head kernels implement binary_crossentropy, mse and mae")
            if self.binary_only and n != "binary_crossentropy":
                raise NotImplementedError(f"{type(self).__name__}: loss {n!r}: {self.binary_only}")
            if task_type == "regression" and n == "binary_crossentropy":
                raise ValueError("binary_crossentropy on a regression task: the cross-entropy of a raw value is undefined; "
                                 "use mse or mae")
        return names

    @staticmethod
    def _accuracy_score(y_true, y_pred):
        from sklearn.metrics import accuracy_score
        return accuracy_score(y_true, np.where(y_pred > 0.5, 1, 0))

    def _get_metrics(self, metrics, set_eps=False):
        from sklearn.metrics import log_loss, mean_squared_error, roc_auc_score
        m = {}
        self.metric_cols = {}
        for name in metrics or []:
            if name in ("binary_crossentropy", "logloss"):
                m[name] = log_loss
            if name == "auc":
                m[name] = roc_auc_score
            if name == "mse":
                m[name] = mean_squared_error
            if name in ("accuracy", "acc"):
                m[name] = self._accuracy_score
            if name in m:
                self.metric_cols[name] = self._metric_columns_of(name)
            self.metrics_names.append(name)
        return m

    def _metric_columns_of(self, name):
        """The columns a metric scores, counted AFTER the task-mode reduction of _metric (mtl: the tasks; msl: the one
        summed column; mtmsl: the two label groups).  None = all of them: every model whose tasks are all binary, as in the
        reference.  Once a task is a regression, auc / acc / logloss score the binary columns and mse the regression
        columns (the reference applies every metric to every column and so cannot score a mixed model at all:
        INTEGRATION.md)."""
        if all(t == "binary" for t in self.task_types):
            return None
        if self.task_name == "msl":
            kinds = [self.task_types[0]]
        elif self.task_name == "mtmsl":
            kinds = [self.task_types[0], self.task_types[self.num_domains]]
        else:
            kinds = list(self.task_types)
        cols = [i for i, k in enumerate(kinds) if k == self.METRIC_KINDS[name]]
        if not cols:
            raise ValueError(f"metric {name!r} scores {self.METRIC_KINDS[name]} tasks and this model has none "
                             f"(task_types = {self.task_types})")
        return cols

    def optimizer(self):
        """The fused optimizer bound to this model's parameter store (created on first use after compile)."""
        store = self._store()
        opt = getattr(self, "_optimizer", None)
        if opt is None or opt.store is not store:
            opt = O.Optimizer(store, self.optim_name, self.optim_config.get("lr", 1e-3), self.table_update)
            self._optimizer = opt
        return opt

    # ---- fused training step ---------------------------------------------------------------------
    def train_step_runner(self, B, use_graph=None, allreduce=None, overlap=None, split_dense=True):
        """Returns a TrainStep for batch size B (cached).  split_dense: run the reference-exact dense table update as
        (untouched rows beside the forward) + (touched rows after the scatter) when possible (trainer.TrainStep)."""
        from ..trainer import TrainStep, resolve_overlap
        overlap = resolve_overlap(overlap)  # (None: the default schedule -- one stream since round 5)
        key = (int(B), bool(self.training))  # BatchNorm follows the MODULE's mode: a step is recorded for one of them
        st = self._caches["steps"].get(key)
        # (the REQUEST is compared, not what the step made of it: TrainStep may lower overlap, and "force" is not True)
        if (st is None or st.store is not self._store() or st.want_overlap != overlap or
                st.want_split != split_dense):
            st = TrainStep(self, B, self.use_hip_graph if use_graph is None else use_graph, allreduce, overlap,
                           split_dense)
            self._caches["steps"][key] = st
        return st

    # ---- fit / evaluate / predict (reference :135-457) -----------------------------------------------
    def _as_matrix(self, x):
        if isinstance(x, dict):
            x = [x[f] for f in self.feature_index]
        cols = []
        for c in x:
            c = np.asarray(c.values if hasattr(c, "values") else c)
            cols.append(c.reshape(len(c), -1))
        return np.concatenate(cols, axis=-1)

    @staticmethod
    def _loader_iter_draw():
        """Every torch DataLoader iterator the reference creates (one per training epoch, one per predict call) takes
        one int64 from the global generator for its base seed; mirroring the draw keeps seeded runs in lock-step."""
        torch.empty((), dtype=torch.int64).random_()

    @classmethod
    def _epoch_permutation(cls, n, shuffle):
        """Same draws as the reference's DataLoader: base-seed draw, then (shuffle=True) RandomSampler draws the
        seed of a private generator and yields torch.randperm(n) from it."""
        cls._loader_iter_draw()
        if not shuffle:
            return torch.arange(n)
        seed = int(torch.empty((), dtype=torch.int64).random_().item())
        g = torch.Generator()
        g.manual_seed(seed)
        return torch.randperm(n, generator=g)

    def fit(self, x=None, y=None, batch_size=None, epochs=1, initial_epoch=0, validation_split=0.0,
            validation_data=None, shuffle=True):
        """Counterpart of BaseModel.fit of the reference (model/basemodel.py:135-371).

        Multi-GPU (after parallel.shard_model; every rank calls fit with the SAME data and the same seed): the epoch
        permutation is dealt to the ranks like torch's DistributedSampler does -- padded with its own first entries to
        a multiple of the world size, rank r takes entries r, r + world, ... -- so every rank runs the same number of
        steps with the same batch sizes; `batch_size` is per rank (global batch = world * batch_size).  Loss and the
        per-step train metrics in the epoch log are averaged over ranks; validation runs on every rank (identical
        results), on the synchronised tables."""
        X_all = self._as_matrix(x)
        n = X_all.shape[0]
        y = np.asarray(y, dtype=np.float32).reshape(n, self.num_tasks)
        do_validation = False
        val_x = val_y = None
        if validation_data:
            if len(validation_data) not in (2, 3):
                raise ValueError("When passing a `validation_data` argument, it must contain either 2 items "
                                 "(x_val, y_val), or 3 items (x_val, y_val, val_sample_weights)")
            val_x, val_y = validation_data[0], validation_data[1]
            val_x = self._as_matrix(val_x)
            val_y = np.asarray(val_y, dtype=np.float32).reshape(val_x.shape[0], self.num_tasks)
            do_validation = True
        elif validation_split and 0.0 < validation_split < 1.0:
            split_at = int(n * (1.0 - validation_split))
            X_all, val_x = X_all[:split_at], X_all[split_at:]
            y, val_y = y[:split_at], y[split_at:]
            n = split_at
            do_validation = True
        if batch_size is None:
            batch_size = 256
        dev = self._store().device
        Xd = torch.as_tensor(X_all, dtype=torch.float32).to(dev)
        yd = torch.as_tensor(y, dtype=torch.float32).to(dev)
        self.train()
        par = getattr(self, "_parallel", None)
        world, rank = (par.world, par.rank) if par is not None else (1, 0)
        n_total, n = n, -(-n // world)  # from here on n = samples of THIS rank per epoch
        steps_per_epoch = (n - 1) // batch_size + 1
        print(dev)
        print("Train on {0} samples, validate on {1} samples, {2} steps per epoch".format(
            n_total, 0 if val_y is None else len(val_y), steps_per_epoch))
        best_auc, early_stop, best_model = 0, 0, None
        # what validation selects on: `auc` when it is compiled (the reference's rule, unchanged).  A model with regression
        # tasks may have no binary column for it (compile refuses `auc` then): it selects on falling `val_mse` when `mse`
        # is compiled, and without either it neither selects nor stops early
        select = "auc"
        if "auc" not in self.metrics and any(t != "binary" for t in self.task_types):
            select = "mse" if "mse" in self.metrics else None
        best_mse = float("inf")
        self.history = []
        pred_epoch = torch.empty((n, self.num_outputs or self.num_tasks), dtype=torch.float32, device=dev)
        for epoch in range(initial_epoch, epochs):
            start_time = time.time()
            profiling.push("epoch %d" % epoch)
            perm = self._epoch_permutation(n_total, shuffle)
            if world > 1:
                pad = n * world - n_total
                if pad:
                    perm = torch.cat([perm, perm[:pad]])
                perm = perm[rank::world].contiguous()
            perm_d = perm.to(dev)
            loss_dev = torch.zeros(1, dtype=torch.float64, device=dev)
            # row-sharded tables: the next batch is staged and ROUTED (distinct rows, owners, count exchange, host read of
            # the split sizes) on a side stream while the current step runs (trainer.TrainStep.prefetch)
            ahead = par is not None and par.mode == "row_sharded"
            for s in range(steps_per_epoch):
                idx = perm_d[s * batch_size:(s + 1) * batch_size]
                step = self.train_step_runner(idx.numel())
                if not step._has_next:
                    torch.index_select(Xd, 0, idx, out=step.plan.X)
                    torch.index_select(yd, 0, idx, out=step.plan.y)
                step.run()
                if ahead and s + 1 < steps_per_epoch:
                    nxt = perm_d[(s + 1) * batch_size:(s + 2) * batch_size]
                    if nxt.numel() == idx.numel():  # (a ragged last batch runs on another plan: it routes itself)
                        step.prefetch(fill=lambda bx, by, nxt=nxt: (torch.index_select(Xd, 0, nxt, out=bx),
                                                                   torch.index_select(yd, 0, nxt, out=by)))
                pred_epoch[s * batch_size:s * batch_size + idx.numel()] = step.plan.prob
                loss_dev += step.plan.loss
            for st in self._caches["steps"].values():
                ops.check_status(st.plan.status, "embedding lookup (nn.Embedding semantics)")
            if world > 1:
                par.comm.all_reduce(loss_dev)
            epoch_logs = {"loss": float(loss_dev.item()) / (n * world), "cka_loss": 0.0}
            # per-batch train metrics, averaged over steps exactly like the reference (:316-337), computed once
            # per epoch on the host instead of once per step
            pred_m = pred_epoch if self.metric_columns is None else pred_epoch[:, list(self.metric_columns)]
            dev_metrics = self._device_batch_metrics(pred_m, yd, perm_d, batch_size)
            pe = ye = None
            for name, fn in self.metrics.items():
                if name in dev_metrics:
                    epoch_logs[name] = dev_metrics[name]
                    continue
                if pe is None:
                    pe = pred_m.cpu().numpy().astype("float64")
                    ye = y[perm.numpy()]
                vals = []
                for s in range(steps_per_epoch):
                    sl = slice(s * batch_size, (s + 1) * batch_size)
                    vals.append(self._metric(fn, ye[sl], pe[sl], self.metric_cols.get(name)))
                epoch_logs[name] = np.sum(vals) / steps_per_epoch
            if world > 1:  # mean over ranks of the per-rank step averages
                names = [m for m in self.metrics]
                t = torch.tensor([epoch_logs[m] for m in names], dtype=torch.float64, device=dev)
                par.comm.all_reduce(t)
                for m, v in zip(names, (t / world).tolist()):
                    epoch_logs[m] = v
            if do_validation:
                # (Reference defect kept OUT: its predict() calls self.eval() and never restores train mode
                # (basemodel.py:231 vs :397), so from the second epoch on the reference trains BatchNorm models with
                # running statistics and returns best_model in eval mode.  Here every epoch trains in train mode; for
                # models without BatchNorm -- every hot-path config -- the two are identical.)
                eval_result = self.evaluate(val_x, val_y, batch_size)
                print(eval_result)
                if select == "auc":
                    better = eval_result.get("auc", 0) > best_auc
                    if better:
                        best_auc = eval_result["auc"]
                elif select == "mse":
                    better = eval_result["mse"] < best_mse
                    if better:
                        best_mse = eval_result["mse"]
                else:
                    better = None
                if better:
                    best_model = copy.deepcopy(self)
                    early_stop = 0
                elif better is not None:
                    early_stop += 1
                for name, result in eval_result.items():
                    epoch_logs["val_" + name] = result
                self.train()
            profiling.pop()
            epoch_time = int(time.time() - start_time)
            print("Epoch {0}/{1}".format(epoch + 1, epochs))
            eval_str = "{0}s - loss: {1: .4f} - cka_loss: {2: .4f}".format(epoch_time, epoch_logs["loss"],
                                                                         epoch_logs["cka_loss"])
            for name in self.metrics:
                eval_str += " - " + name + ": {0: .4f}".format(epoch_logs[name])
            if do_validation:
                for name in self.metrics:
                    eval_str += " - val_" + name + ": {0: .4f}".format(epoch_logs["val_" + name])
            print(eval_str)
            self.history.append(epoch_logs)
            if early_stop >= self.optim_config.get("early_stop", 3):
                break
        self.flush_tables()  # multi-GPU: leave every rank's full tables equal to the trained state (collective)
        return best_model if best_model is not None else self  # reference D7: unbound when nothing improved

    def _device_batch_metrics(self, pred, yd, perm_d, batch_size):
        """Per-batch `auc` / `acc` averaged over the steps of an epoch, computed where the predictions already are
        (reference: sklearn on the host after every step, model/basemodel.py:316-337).  Same task-mode reductions as
        _metric: msl -> (label 0, sum of the heads); mtmsl -> per label group; mtl -> sklearn's multilabel behaviour
        (macro-average AUC over tasks, exact-match accuracy).  Returns {} when a metric cannot be done on the device
        (batches over 4096 rows): the caller then falls back to the host path."""
        want = [m for m in self.metrics if m in ("auc", "acc", "accuracy", "mse")]
        # batches above 4096 rows: one workgroup cannot sort them (ops.auc_segments); with the device_metrics switch on
        # they take the multi-workgroup sort (ops.auc_sorted), otherwise the host path as before
        big = batch_size > 4096
        if not want or (big and not getattr(self, "device_metrics", False)) or not pred.is_cuda:
            return {}
        ye = yd.index_select(0, perm_d)
        if big:  # (the heads of a group are summed in float64, as on the host: _order_scores)
            yt, pt = self._device_columns(ye, pred)
        elif self.task_name == "msl":
            yt, pt = ye[:, :1], pred.sum(-1, keepdim=True)
        elif self.task_name == "mtmsl":
            D = self.num_domains
            yt = ye[:, [0, D]]
            pt = torch.stack([pred[:, :D].sum(-1), pred[:, D:].sum(-1)], -1)
        else:
            yt, pt = ye, pred
        n = pt.shape[0]
        steps = (n - 1) // batch_size + 1
        out = {}

        def columns(name):  # (the metric's own columns once a task is a regression: _metric_columns_of)
            cols = getattr(self, "metric_cols", {}).get(name)
            if cols is None:
                return yt.contiguous(), pt.contiguous()
            return yt[:, cols].contiguous(), pt[:, cols].contiguous()

        def step_means(v):  # [n] float64 -> mean over steps of the per-batch means
            seg = torch.arange(n, device=v.device) // batch_size
            per = torch.zeros(steps, dtype=torch.float64, device=v.device).index_add_(0, seg, v)
            cnt = torch.zeros(steps, dtype=torch.float64, device=v.device).index_add_(0, seg, torch.ones_like(v))
            return float((per / cnt).sum().item()) / steps

        if "auc" in want:
            ya, pa = columns("auc")
            # [steps, C]; NaN = single-class batch
            if big and pa.dtype == torch.float64:
                pa = torch.stack([self._order_scores(pa[:, c]) for c in range(pa.shape[1])], -1).contiguous()
            a = ops.auc_sorted(pa, ya, seg=batch_size) if big else ops.auc_segments(pa, ya, batch_size)
            out["auc"] = float(a.mean(1).sum().item()) / steps  # macro average over columns, mean over steps
        for name in ("acc", "accuracy"):
            if name in want:
                ya, pa = columns(name)
                out[name] = step_means(((pa > 0.5) == (ya > 0.5)).all(1).to(torch.float64))  # exact match over the columns
        if "mse" in want:  # sklearn's mean_squared_error: the mean over samples and columns
            ya, pa = columns("mse")
            out["mse"] = step_means(((pa.double() - ya.double()) ** 2).mean(1))
        return out

    def _metric(self, fn, y_true, y_pred, cols=None):
        """Task-mode specific metric reduction (reference :320-331, :383-392); cols: _metric_columns_of."""
        try:
            if self.task_name == "msl":
                return fn(y_true[:, 0], y_pred.sum(-1))
            if self.task_name == "mtmsl":
                D = self.num_domains
                y_true = y_true[:, [0, D]]
                y_pred = np.stack([y_pred[:, :D].sum(-1), y_pred[:, D:].sum(-1)], -1)
            if cols is not None:
                y_true, y_pred = y_true[:, cols], y_pred[:, cols]
                if len(cols) == 1:
                    y_true, y_pred = y_true[:, 0], y_pred[:, 0]
            return fn(y_true, y_pred)
        except ValueError:  # a batch with a single class has no AUC; the reference would raise here
            return float("nan")

    @staticmethod
    def _order_scores(s64):
        """fp32 scores with exactly the order and the ties of a float64 device vector: its dense ranks, written as the bit
        patterns of increasing normal floats.  The host path ranks the float64 sum of an msl / mtmsl group's heads; rounding
        that sum to fp32 would merge scores that differ, and one merged (positive, negative) pair moves the AUC by
        1 / (2 P N).  mml_auc_sorted orders by bit pattern, so ranks up to 2^31 - 2^24 are exact.  A NaN or infinite score
        stays NaN (torch.unique would rank it like any value): the kernel then flags it and the problem's AUC is NaN, as
        sklearn's refusal makes it on the host."""
        _, inv = torch.unique(s64, sorted=True, return_inverse=True)
        ranks = (inv + 0x00800000).to(torch.int32).view(torch.float32)
        return torch.where(torch.isfinite(s64), ranks, torch.full_like(ranks, float("nan")))

    def _device_columns(self, yd, pred):
        """The task-mode reduction of _metric on device tensors: labels [n, C] float32 and scores [n, C] (float64 where a
        column is a sum of heads, as on the host, else the fp32 predictions)."""
        if self.task_name == "msl":
            return yd[:, :1], pred.double().sum(-1, keepdim=True)
        if self.task_name == "mtmsl":
            D = self.num_domains
            p64 = pred.double()
            return yd[:, [0, D]], torch.stack([p64[:, :D].sum(-1), p64[:, D:].sum(-1)], -1)
        return yd, pred

    def _evaluate_device(self, x, y, batch_size, domain_mask):
        """evaluate() with the device_metrics switch on: the predictions stay in HBM; auc = macro average over the columns
        of ops.auc_sorted over the whole set, acc / mse as in _device_batch_metrics.  logloss keeps the host path
        (O(n), and the clip rule is sklearn's)."""
        pred_d, _ = self._predict_device(x, batch_size, domain_mask)
        if self.metric_columns is not None:
            pred_d = pred_d[:, list(self.metric_columns)]
        n = pred_d.shape[0]
        y = np.asarray(y).reshape(n, -1)
        yd = torch.as_tensor(y, dtype=torch.float32).to(pred_d.device)
        yt, pt = self._device_columns(yd, pred_d)
        out, host_pred = {}, None
        for name, fn in self.metrics.items():
            cols = self.metric_cols.get(name)
            # (msl has ONE summed column and _metric never selects from it: the same here)
            ya, pa = (yt, pt) if cols is None or self.task_name == "msl" else (yt[:, cols], pt[:, cols])
            if name == "auc":
                if pa.dtype == torch.float64:
                    pa = torch.stack([self._order_scores(pa[:, c]) for c in range(pa.shape[1])], -1)
                a = ops.auc_sorted(pa.contiguous(), ya.contiguous(), seg=0)  # [1, C]; NaN = single-class column
                out[name] = float(a.mean().item())
            elif name in ("acc", "accuracy"):
                out[name] = int(((pa > 0.5) == (ya > 0.5)).all(1).sum().item()) / n  # exact match over the columns
            elif name == "mse":
                out[name] = float(((pa.double() - ya.double()) ** 2).mean(0).mean().item())
            else:
                if host_pred is None:
                    host_pred = pred_d.cpu().numpy().astype("float64")
                out[name] = self._metric(fn, y, host_pred, cols)
        return out

    def evaluate(self, x, y, batch_size=256, domain_mask=None):
        # (a model that is not on a GPU keeps the host path, like _device_batch_metrics; it cannot predict there anyway)
        if getattr(self, "device_metrics", False) and self._store().device.type == "cuda":
            return self._evaluate_device(x, y, batch_size, domain_mask)
        pred = self.predict(x, batch_size, domain_mask)
        if self.metric_columns is not None:  # (the reference scores all columns here and raises for ESCM: model/escm.py)
            pred = pred[:, list(self.metric_columns)]
        y = np.asarray(y).reshape(len(pred), -1)
        return {name: self._metric(fn, y, pred, self.metric_cols.get(name)) for name, fn in self.metrics.items()}

    def predict(self, x, batch_size=256, domain_mask=None):
        """float64 [N,T] predictions -- probabilities, raw values in the columns of regression tasks (reference :395-457).  Like the reference's loop (:436-437) the heads
        are NOT masked here; pass a mask to forward() directly for masked outputs."""
        pred, layers = self._predict_device(x, batch_size, domain_mask)
        pred = pred.cpu().numpy().astype("float64")
        if self.save_layer_output:
            return pred, {k: np.concatenate(v).astype("float64") for k, v in layers.items()}
        return pred

    def _predict_device(self, x, batch_size=256, domain_mask=None):
        """The predict loop: float32 [N,T] predictions on the device, and the collected layer outputs (host lists)."""
        was_training = self.training
        self.eval()
        X = x if isinstance(x, np.ndarray) and x.ndim == 2 else self._as_matrix(x)
        dev = self._store().device
        Xd = torch.as_tensor(X, dtype=torch.float32).to(dev)
        self._loader_iter_draw()
        outs, layers = [], {}
        self._defer_status = True
        try:
            with torch.no_grad():
                for s in range(0, Xd.shape[0], batch_size):
                    outs.append(self.forward(Xd[s:s + batch_size], None))
                    if self.save_layer_output:
                        for k, v in self.layer_output_dict.items():
                            layers.setdefault(k, []).append(v.cpu().numpy())
        finally:
            self._defer_status = False
        for pl in self._caches["plans"].values():  # out-of-range indices of ANY batch are sticky in the plan's status word
            ops.check_status(pl.status, "embedding lookup (nn.Embedding semantics)")
        pred = torch.cat(outs)
        self.train(was_training)
        return pred, layers
