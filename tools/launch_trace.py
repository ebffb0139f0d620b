"""What the ViT block's Python code asks of the library, in order -- the Python-side counterpart of obj_isa_diff.py: the check that a refactor of
the model code left every launch, its arguments, its stream and the stream ordering alone, and the results bit for bit.

    python tools/launch_trace.py TREE OUT.txt          one run (fresh process) importing alpro_amd and tests from TREE
    python tools/launch_trace.py --diff OLD1 OLD2 NEW  OLD run twice (what differs between them is not deterministic) against NEW

One line per library call (C name, every non-pointer argument, pointers as null / ptr, GemmDesc fields, the stream as a label numbered by first
appearance) and per record_event / wait_event; behind each configuration the SHA-256 of every result and, for training, the peak allocation.
ALPRO_HIP_LIB names the library when TREE has none built."""
import copy
import ctypes
import hashlib
import itertools
import os
import sys


def _diff(old1, old2, new):
    def read(path):
        cfgs, cur = {}, None
        for line in open(path):
            if line.startswith("## "):
                cur = cfgs.setdefault(line[3:].strip(), ([], []))
            else:
                cur[line.startswith(("sha ", "peak "))].append(line)
        return cfgs
    a, b, c = read(old1), read(old2), read(new)
    noisy = sorted(k for k in a if a[k][1] != b.get(k, a[k])[1])
    bad_trace = sorted(k for k in set(a) | set(c) if a.get(k, (None,))[0] != c.get(k, (None,))[0])
    bad_res = sorted(k for k in a if k not in noisy and k in c and a[k][1] != c[k][1])
    print("configurations: %d old, %d new; launch / event lines: %d old, %d new" % (len(a), len(c), sum(len(v[0]) for v in a.values()), sum(len(v[0]) for v in c.values())))
    print("not deterministic between the two old runs (excluded from the result comparison): %s" % (noisy or "none"))
    print("trace lines differ: %s" % (bad_trace or "none"))
    print("result hashes / peak allocation differ: %s" % (bad_res or "none"))
    return 1 if (bad_trace or bad_res) else 0


if sys.argv[1] == "--diff":
    sys.exit(_diff(*sys.argv[2:5]))
TREE, OUT = os.path.abspath(sys.argv[1]), open(sys.argv[2], "w")
sys.path.insert(0, TREE)
import torch  # noqa: E402
from alpro_amd import config as rt, hip  # noqa: E402
from alpro_amd.modeling.timesformer import vit  # noqa: E402
from tests.test_hip_ops import rnd  # noqa: E402
from tests.test_host_cpu import VENC  # noqa: E402
from tests.test_vit_attn_dropout import D, _block, _fix_drop_path  # noqa: E402

assert os.path.abspath(vit.__file__).startswith(TREE), vit.__file__
labels = {"s": {}, "e": {}}


def label(kind, key):
    return labels[kind].setdefault(key, "%s%d" % (kind, len(labels[kind])))


def fmt(v, ctype=None):
    if isinstance(v, ctypes.Array) or hasattr(v, "_obj"):   # GemmDesc by reference / a table of them
        return " ".join("{%s}" % " ".join("%s=%s" % (n, fmt(getattr(d, n), t)) for n, t in d._fields_) for d in (v if isinstance(v, ctypes.Array) else [v._obj]))
    if v is None or ctype is ctypes.c_void_p or isinstance(v, ctypes.c_void_p):
        return "ptr" if getattr(v, "value", v) else "null"
    return repr(v.value if hasattr(v, "value") else v)


class Recorder:
    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        types = fn.argtypes or []
        if not types or types[-1] is not ctypes.c_void_p:   # no stream argument: queries, options
            return fn

        def call(*args):
            OUT.write("%s %s %s\n" % (name, " ".join(fmt(a, t) for a, t in zip(args[:-1], types)), label("s", getattr(args[-1], "value", args[-1]) or 0)))
            return fn(*args)
        return call


def patch_events():
    rec, wait = torch.cuda.Stream.record_event, torch.cuda.Stream.wait_event

    def record_event(self, event=None):
        ev = rec(self, event)
        OUT.write("record_event %s %s\n" % (label("s", self.cuda_stream), label("e", ev)))
        return ev

    def wait_event(self, event):
        OUT.write("wait_event %s %s\n" % (label("s", self.cuda_stream), label("e", event)))
        return wait(self, event)
    torch.cuda.Stream.record_event, torch.cuda.Stream.wait_event = record_event, wait_event


def config(name, run, training):
    """run() -> {name: tensor}; its launches, then the hashes of what it returned."""
    labels["s"].clear(), labels["e"].clear()
    OUT.write("## %s\n" % name)
    rt.seed_dropout(4242)
    torch.cuda.reset_peak_memory_stats()
    res = run()
    vit.join_cls_chain(torch.device("cuda"))
    torch.cuda.synchronize()
    for k in sorted(res):
        OUT.write("sha %s %s\n" % (k, hashlib.sha256(res[k].detach().contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()))
    if training:
        OUT.write("peak %d\n" % torch.cuda.max_memory_allocated())


def grads(m):
    return {"grad " + n: p.grad for n, p in m.named_parameters() if p.grad is not None}


def block_level():
    pristine = {ad: _block(ad) for ad in (0.0, 0.1)}   # never run: every configuration starts from a copy with cold operand caches
    for (B, T, W), mode, merge, cp, cs, defer, fuse, ad, train, path in itertools.product(
            ((2, 2, 4), (2, 3, 3)), ("fp32", "fp16", "bf16"), (True, False), "01", "01", (False, True), "01", (0.0, 0.1), (True, False),
            ("forward", "forward_train", "forward_cls")):
        if path == "forward_cls" and train:   # an eval-mode path
            continue
        N = W * W
        blk = copy.deepcopy(pristine[ad]).train(train)
        blk.merge_temporal_proj = merge
        _fix_drop_path(blk, B, T, N)
        x, dout = rnd(B, 1 + N * T, D, seed=610).cuda(), rnd(B, 1 + N * T, D, seed=611).cuda()
        rt.set_cls_stream(cs), rt.set_defer_temporal_add(defer), rt.set_fuse_temporal_attention(fuse)

        def run():
            with rt.use_compute_dtype(mode), rt.use_cls_precise(cp), torch.no_grad():
                if path != "forward_train":
                    return {"out": getattr(blk, path)(x.clone(), B, T, W)}
                out, sv = blk.forward_train(x.clone(), B, T, W)
                return dict(grads(blk), out=out, dx=blk.backward(sv, dout.clone())[0])
        config("block B=%d T=%d W=%d %s merge=%d cls_precise=%s cls_stream=%s defer=%d fuse=%s attn_drop=%s train=%d %s"
               % (B, T, W, mode, merge, cp, cs, defer, fuse, ad, train, path), run, path == "forward_train")


def encoder_level():
    B, T = 2, 2
    torch.manual_seed(21)
    enc = vit.TimeSformer(dict(VENC, num_frm=T, drop_path_rate=0.1), input_format="RGB").cuda()
    x = torch.randn(B, 3, T, 224, 224, device="cuda")
    dout = torch.randn(B, 197, 768, device="cuda") * 1e-2
    rt.set_cls_stream("infer"), rt.set_defer_temporal_add(True), rt.set_fuse_temporal_attention("infer")
    for mode in ("fp16", "bf16"):
        for split, path in itertools.product("01", ("forward_features", "forward_cls")):
            def run():
                rt.set_split_streams(split)
                with rt.use_compute_dtype(mode), torch.no_grad():
                    return {"out": getattr(enc.eval(), path)(x)}
            config("encoder %s split_streams=%s %s" % (mode, split, path), run, False)

        def run():
            torch.manual_seed(5)   # the drop-path draw
            for p in enc.parameters():
                p.grad = None
            with rt.use_compute_dtype(mode), torch.enable_grad(), rt.loss_scaling(True):
                y = enc.train().forward_features(x)
                (y * dout).sum().backward()
            return dict(grads(enc), out=y)
        config("encoder %s autograd forward_features + backward" % mode, run, True)


hip._lib = Recorder(hip.load())
patch_events()
block_level()
encoder_level()
OUT.close()
