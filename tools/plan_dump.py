#!/usr/bin/env python3
"""Canonical text of a recorded step: every call list of the plan and of the step runner, entry by entry.

    python tools/plan_dump.py --workload mmoe_ae30 --batch 65536 [--table-update dense_exact] [--scatter-mode atomic]
                              [--gemm-mode N] [--streams 2] [--vocab-scale 0.2] [--split-dense force|off]
                              [--pcgrad total|per_task] [--model-kw KEY=VALUE ...] [--infer] [--out FILE]

Two trees record the same step iff their dumps are equal: the before / after check of a change to engine.py or
trainer.py (diff the two files).  Per entry: the function's name, its meta without pointers, its scalar arguments, and
every ctypes descriptor walked field by field (fields that are zero are left out).  Device addresses differ from run to
run, so each is replaced by an ordinal in order of first appearance (`@3`); a bare integer argument counts as an address
from 2^32 on -- the rule of trainer.fork_conflicts.  Records plans on the GPU, runs no step.
The first line names every option of THIS copy of the tool (pcgrad= and split_dense= since they exist), so a dump differs
in that line from one an older copy wrote: make both sides of a comparison with one copy (it runs in older trees)."""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import mmlrec_amd  # noqa: E402,F401
from mmlrec_amd import _lib as L, engine as E, workloads as W  # noqa: E402

# (a tree that predates engine.call_meta can still be dumped: the "before" side of the change that introduced it)
call_meta = getattr(E, "call_meta", lambda c: c[-1] if isinstance(c[-1], dict) else {})
PLAN_LISTS = ("fwd", "head_infer", "head_train", "head_bwd", "bwd", "bwd_tail", "head_side", "bwd_side")
STEP_SEGMENTS = ("pre", "early", "front", "front_b", "side_a", "sideq", "tail", "whole")


class Canon:
    def __init__(self):
        self.addr = {}

    def ptr(self, a):
        if not a:
            return "0"
        return "@%d" % self.addr.setdefault(int(a), len(self.addr))

    def scalar(self, v):
        if isinstance(v, bool) or v is None:
            return repr(v)
        if isinstance(v, int):
            return self.ptr(v) if v >= (1 << 32) else str(v)
        if isinstance(v, float):
            return repr(v)
        if isinstance(v, (bytes, str)):
            return repr(v)
        if isinstance(v, torch.Tensor):
            return "tensor(%s %s %s)" % (tuple(v.shape), str(v.dtype).replace("torch.", ""), self.ptr(v.data_ptr()))
        return None

    def value(self, v):
        """One argument or descriptor field as text ('' = zero / empty, left out of a descriptor)."""
        s = self.scalar(v)
        if s is not None:
            return s
        if hasattr(v, "_obj"):  # ctypes.byref(x)
            return self.value(v._obj)
        if isinstance(v, C.Structure):
            parts = []
            for name, *_ in v._fields_:
                t = self.value(getattr(v, name))
                if t not in ("", "0", "0.0", "None", "[]", "{}"):
                    parts.append("%s=%s" % (name, t))
            return "{" + " ".join(parts) + "}"
        if isinstance(v, C.Array):
            items = [self.value(x) for x in v]
            while items and items[-1] in ("", "0", "0.0", "None", "[]", "{}"):
                items.pop()
            return "[" + ", ".join(items) + "]"
        if isinstance(v, C._Pointer) or isinstance(v, (C.c_void_p, C.c_char_p)):
            return self.ptr(C.cast(v, C.c_void_p).value)
        if isinstance(v, C._SimpleCData):
            return self.value(v.value)
        if isinstance(v, (tuple, list)):
            return "(" + ", ".join(self.value(x) for x in v) + ")"
        return "<%s>" % type(v).__name__

    def meta(self, m):
        out = []
        for k in sorted(m):
            if k == "ptrs":
                out.append("ptrs=[%s]" % ", ".join(self.ptr(p) for p in m[k]))
            elif k == "need":
                out.append("need=[%s]" % ", ".join("%s->%s" % (self.value(t), self.value(s)) for t, s in m[k]))
            else:
                out.append("%s=%s" % (k, self.value(m[k])))
        return " ".join(out)

    def entry(self, c):
        if c[0] is E.PY or c[0] is E.INLINE:
            kind = "PY" if c[0] is E.PY else "INLINE"
            return "%s %s | %s" % (kind, getattr(c[1], "__qualname__", type(c[1]).__name__), self.meta(call_meta(c)))
        return "%s | %s | %s" % (c[0].__name__, self.meta(call_meta(c)), " ; ".join(self.value(a) for a in c[1]))

    def calls(self, title, calls, out):
        out.append("== %s (%d)" % (title, len(calls)))
        out.extend("  " + self.entry(c) for c in calls)


def dump(args):
    dev = torch.device("cuda:0")
    lib = L.load()
    if args.gemm_mode is not None:
        lib.mml_gemm_set_mode(args.gemm_mode)
    kw = dict(table_update=args.table_update)
    if args.scatter_mode:
        kw["scatter_mode"] = args.scatter_mode
    if args.pcgrad:  # (the workload's model as model_name "pcg": PCGrad over its tasks)
        kw.update(seed=0, model_name="pcg")
    for item in args.model_kw:  # (forwarded to workloads.build_model: the value as JSON, else as the string it is)
        key, _, text = item.partition("=")
        try:
            kw[key] = json.loads(text)
        except ValueError:
            kw[key] = text
    model, cfg, _, _ = W.build_model(args.workload, dev, vocab_scale=args.vocab_scale, **kw)
    if args.pcgrad:
        model.optim_config["pcgrad_objectives"] = args.pcgrad
    oc = cfg["optim_config"]
    model.compile(oc["optimizer"], oc["loss"], oc["metrics"])
    canon, out = Canon(), []
    out.append("# %s" % " ".join("%s=%s" % kv for kv in sorted(vars(args).items()) if kv[0] != "out"))
    if args.infer:
        model.eval()
        plan = model._get_plan(args.batch, False, False)
        for name in PLAN_LISTS:
            canon.calls("plan." + name, getattr(plan, name), out)
        return out
    model.train()
    step = model.train_step_runner(args.batch, overlap=(args.streams == 2),
                                   split_dense={"default": True, "force": "force", "off": False}[args.split_dense])
    for name in PLAN_LISTS:
        canon.calls("plan." + name, getattr(step.plan, name), out)
    for name in ("pre", "early", "mlp", "tables"):
        canon.calls("opt_split." + name, step.opt_split[name], out)
    for name in STEP_SEGMENTS:
        seg = getattr(step, name, None)
        if seg is None:
            out.append("== step.%s none" % name)
            continue
        for i, (kind, item, _) in enumerate(seg.parts):
            canon.calls("step.%s[%d] %s" % (name, i, kind), item if kind == "c" else [item], out)
    fork = getattr(step, "inner_fork", None)
    canon.calls("step.inner_fork", fork.calls if fork is not None else [], out)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--workload", default="mmoe_ae30")
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--table-update", default="dense_exact")
    ap.add_argument("--scatter-mode", default=None, choices=["atomic", "deterministic"])
    ap.add_argument("--gemm-mode", type=int, default=None, help="mml_gemm_set_mode before the model is built")
    ap.add_argument("--streams", type=int, default=1, choices=[1, 2])
    ap.add_argument("--vocab-scale", type=float, default=1.0)
    ap.add_argument("--split-dense", default="default", choices=["default", "force", "off"],
                    help="the split_dense request of train_step_runner: True, 'force' or False")
    ap.add_argument("--pcgrad", default=None, choices=["total", "per_task"],
                    help="build the workload as model_name='pcg' with these pcgrad_objectives")
    ap.add_argument("--model-kw", action="append", default=[], metavar="KEY=VALUE",
                    help="a keyword for workloads.build_model (repeatable), e.g. dnn_use_bn=true, dnn_activation=prelu")
    ap.add_argument("--infer", action="store_true", help="the forward-only plan instead of a training step")
    ap.add_argument("--out", default=None, help="write here instead of stdout")
    args = ap.parse_args()
    text = "\n".join(dump(args)) + "\n"
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
