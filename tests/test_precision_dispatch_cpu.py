"""Which ``ops`` call a pass issues, in which order, with which packed weights.

``nerf/network_tcnn_semantics.py`` and ``nerf/renderer_semantics.py`` choose the
arithmetic of a pass (fp32, fp16, fp16 with the fp16 table, bf16x3, f16x2, the
training modes) and with it the weight packs, the sigma-MLP op, the render op and
the composite op.  Here every ``ops`` function the two modules call is replaced by
a recording stub that returns CPU tensors of the right shapes; the pack stubs
return tagged tensors, so a trace line says WHICH pack reached WHICH argument and
whether a pack call got a buffer to reuse (``out=given``).  The whole traces are
compared with tests/golden/dispatch_trace.json, recorded with ``record()`` below
(``PYTHONPATH=. python tests/test_precision_dispatch_cpu.py`` from the repository
root; a re-recording on an unchanged dispatch is byte-identical).  No GPU needed: the built
library is used for ``ucsa_grid_init`` in the constructor only.
"""
import contextlib
import functools
import inspect
import json
import os
import types

import pytest
import torch

from ucsa_neural_rendering_amd import _lib, ops

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden",
                      "dispatch_trace.json")

pytestmark = pytest.mark.skipif(
    not os.path.exists(_lib.LIB_PATH),
    reason="libucsa_hip.so is not built (SemanticNeRFNetwork() needs ucsa_grid_init)")

N, T, C = 8, 4, 5
N_INFER, INFER_CHUNK = 20, 8          # three chunks: 8 + 8 + 4 rays

PACK_DTYPE = {"mlp_pack": torch.float32, "mlp_pack_t": torch.float32,
              "mlp_pack_f16": torch.float16, "mlp_pack_t_f16": torch.float16,
              "mlp_pack_x3": torch.bfloat16, "mlp_pack_t_x3": torch.bfloat16,
              "mlp_pack_h2": torch.float16, "table_to_half": torch.float16}
KIND = {_lib.MLP_SIGMA: "sigma", _lib.MLP_COLOR: "color", _lib.MLP_SEM: "sem"}
PRESENCE = ("out", "range_bits", "scratch")      # recorded as given / none
FLOATS = ("rec_scale", "f16_scale")              # flag-like floats, recorded by value
SILENT = {"shade_bwd_split", "render_workspace_bytes"}     # answered, not recorded


def _z(*shape, **kw):
    return torch.zeros(*shape, **kw)


def _five(a):
    n, tt = a["z_c"].shape[0], a["z_c"].shape[1] + (0 if a["z_f"] is None else a["z_f"].shape[1])
    return (_z(n, 3), _z(n), _z(n, a["n_classes"]), _z(n, tt, dtype=torch.int32), _z(n, tt))


def _sigma(a):
    return _z(a["feat"].shape[1], 16), _z(a["feat"].shape[1])


def _composite_bwd(a):
    n, tc = a["z_c"].shape
    tf = 0 if a["z_f"] is None else a["z_f"].shape[1]
    return (_z(n * tc, 16), _z(n * tf, 16) if tf else None, _z(1, 7168),
            _z(1, 1024 + 1024 * ((a["n_classes"] + 15) // 16)))


RETURNS = {
    "near_far_from_aabb": lambda a: (_z(a["rays_o"].shape[0]), _z(a["rays_o"].shape[0])),
    "sample_coarse": lambda a: _z(a["nears"].shape[0], a["T"]),
    "hashgrid_encode_rays": lambda a: _z(a["grid"].n_levels, a["z"].numel(), 2,
                                         dtype=a["table"].dtype),
    "sigma_mlp_fwd": _sigma, "sigma_mlp_fwd_f16": _sigma, "sigma_mlp_fwd_x3": _sigma,
    "sigma_mlp_fwd_h2": _sigma,
    "resample": lambda a: _z(a["z"].shape[0], a["u"].shape[1]),
    "composite_fwd": lambda a: _five(a) if a["want_aux"] else _five(a)[:3],
    "composite_train_fwd_x3": _five,
    "composite_bwd": _composite_bwd,
    "sigma_mlp_bwd": lambda a: (torch.zeros_like(a["feat"]), _z(1, 3072)),
    "reduce_partials": lambda a: None,
    "hashgrid_bwd_rays": lambda a: None,
    "hashgrid_bwd_rays_merged": lambda a: None,
    "hashgrid_bwd_rays_det": lambda a: _z(1, dtype=torch.int64) if a["fix"] is None else a["fix"],
    "hashgrid_bwd_det_finish": lambda a: None,
    "render_fused_fwd": lambda a: (_z(a["rays_o"].shape[0], 3), _z(a["rays_o"].shape[0]),
                                   _z(a["rays_o"].shape[0], a["n_classes"]), {}),
    "render_fused_bwd": lambda a: None,
    "render_fwd": lambda a: None, "render_fwd_f16": lambda a: None,
    "render_fwd_f16_h16": lambda a: None, "render_fwd_x3": lambda a: None,
    "render_fwd_h2": lambda a: None, "render_view": lambda a: None,
    "render_workspace_bytes": lambda a: 64,
}


class Tagged:
    def __init__(self, tag):
        self._tag = tag


class Recorder:
    """The stubs and the trace they write."""

    def __init__(self, net):
        self.calls = []
        self.split = True
        self.params = {net.encoder.params.data_ptr(): "param:grid",
                       net.sigma_net.params.data_ptr(): "param:sigma",
                       net.color_net.params.data_ptr(): "param:color",
                       net.semantics_net.params.data_ptr(): "param:sem"}

    def label(self, v):
        tag = getattr(v, "_tag", None)
        if tag is None and torch.is_tensor(v):
            tag = self.params.get(v.data_ptr())
        return tag

    def line(self, op, args):
        parts = [op]
        for k, v in args.items():
            if k in PRESENCE:
                parts.append(f"{k}={'none' if v is None else 'given'}")
            elif isinstance(v, (bool, str)):
                parts.append(f"{k}={v}")
            elif k in FLOATS:
                parts.append(f"{k}={float(v)!r}")
            elif self.label(v) is not None:
                parts.append(f"{k}={self.label(v)}")
            elif op in PACK_DTYPE and k in ("params", "table"):
                parts.append(f"{k}=copy")       # a tensor made from the parameters
        return " ".join(parts)

    def stub(self, name):
        sig = inspect.signature(getattr(ops, name))

        def call(*args, **kwargs):
            bound = sig.bind(*args, **kwargs)
            bound.apply_defaults()
            a = bound.arguments
            if name not in SILENT:
                self.calls.append(self.line(name, a))
            if name == "shade_bwd_split":
                return self.split
            if name == "train_packs":
                return Tagged("packs(" + ",".join(self.label(v) or "-" for v in a.values()) + ")")
            if name in PACK_DTYPE:
                if a["out"] is not None:
                    return a["out"]
                out = torch.zeros(4, dtype=PACK_DTYPE[name])
                out._tag = name + (":" + KIND[a["kind"]] if "kind" in a else "")
                if self.label(a.get("params", a.get("table"))) is None:
                    out._tag += ":copy"
                return out
            return RETURNS[name](a)
        return call

    def take(self):
        calls, self.calls = self.calls, []
        return calls


STUBBED = sorted(set(RETURNS) | set(PACK_DTYPE) | {"train_packs", "shade_bwd_split"})


class ReachedLibrary(Exception):
    pass


def install(mp, net):
    """Stub the ops, fake the three things that need a device, and make the
    library unreachable so that an op without a stub cannot go unnoticed."""
    rec = Recorder(net)
    for name in STUBBED:
        mp.setattr(ops, name, rec.stub(name))

    def boom(*a, **k):
        raise ReachedLibrary("an op without a stub reached lib()")
    for m in vars(ops).values():
        if inspect.ismodule(m) and m.__name__.startswith(ops.__name__ + ".") and hasattr(m, "lib"):
            mp.setattr(m, "lib", boom)
    mp.setattr(ops, "lib", boom)
    mp.delenv("UCSA_H2_GUARD", raising=False)
    # the range word lives in pinned host memory: a plain int32 tensor here
    mp.setattr(net, "_h2_flag", lambda name, device: net._h2_flags.setdefault(
        name, torch.zeros(1, dtype=torch.int32)))
    # the render workspace is keyed by the caller's stream
    mp.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(cuda_stream=0))
    mp.setattr(torch.cuda, "stream", lambda stream: contextlib.nullcontext())
    return rec


@functools.lru_cache(maxsize=None)
def _net():
    from ucsa_neural_rendering_amd.nerf.network_tcnn_semantics import SemanticNeRFNetwork
    return SemanticNeRFNetwork(num_semantic_classes=C, seed=0)


DEFAULTS = dict(train_precision="fp32", bwd_precision="bf16x2", train_fwd_f16x2=True,
                fused_train_calls=True, deterministic=False, grid_records_packed=True,
                grid_bwd_merged=True, h2_guard="weights", f16_grid_records=True,
                f16_bwd_scale=1024.0, precision="fp32", fp16_table=False, hip_pipeline=True,
                hip_streams=1, hip_ray_chunk=INFER_CHUNK, hip_pipeline_rays=INFER_CHUNK)


def fresh(net, **settings):
    """The shared network with empty caches and the given switches."""
    for k, v in dict(DEFAULTS, **settings).items():
        setattr(net, k, v)
    net._packed = {}
    net._h2_seen, net._h2_flags, net._h2_scratch = {}, {}, {}
    net._h2_eval_pending = False
    net._ws = None
    return net


def train_cases():
    """id -> (settings, t, shade_bwd_split): the 44 combinations and the switches
    flipped once each."""
    cases = {}
    modes = [dict(train_precision=p) for p in ("fp32", "fp16", "tcnn")]
    modes += [dict(train_precision="bf16x3", bwd_precision=b, train_fwd_f16x2=h, fused_train_calls=f)
              for b in ("bf16x2", "fp32") for h in (True, False) for f in (True, False)]
    for m in modes:
        for det in (False, True):
            for t in (4, 0):
                s = dict(m, deterministic=det)
                cases["train/" + ",".join(f"{k}={v}" for k, v in s.items()) + f",t={t}"] = (s, t, True)
    x3 = dict(train_precision="bf16x3")
    cases["train/bf16x3,shade_bwd_split=False,t=4"] = (x3, 4, False)
    cases["train/bf16x3,grid_records_packed=False,t=4"] = (dict(x3, grid_records_packed=False), 4, True)
    cases["train/bf16x3,grid_bwd_merged=False,t=4"] = (dict(x3, grid_bwd_merged=False), 4, True)
    cases["train/bf16x3,h2_guard=off,t=4"] = (dict(x3, h2_guard="off"), 4, True)
    return cases


def infer_cases():
    rows = [("fp32", False), ("fp16", False), ("fp16", True), ("bf16x3", False), ("f16x2", False)]
    return {f"infer/{p}{'+fp16_table' if h else ''},pipeline={pipe}":
            dict(precision=p, fp16_table=h, hip_pipeline=pipe)
            for p, h in rows for pipe in (True, False)}


def _rays(n, t):
    g = torch.Generator().manual_seed(1)
    o, d = torch.rand(n, 3, generator=g), torch.rand(n, 3, generator=g)
    return o, d, torch.ones(n), [-1.0, -1.0, -1.0, 1.0, 1.0, 1.0], (torch.rand(n, t, generator=g) if t else None)


def is_pack(line):
    return line.split(" ", 1)[0] in PACK_DTYPE


def run_train(net, rec, settings, t, split):
    """Three steps: pack; pack nothing; repack everything after an update."""
    fresh(net, **settings).train()
    rec.split = split
    o, d, nrm, aabb, u = _rays(N, t)
    traces = []
    for step in range(3):
        if step == 2:
            with torch.no_grad():
                for p in net.parameters():
                    p.add_(0)                   # bumps _version, like an optimizer step
        image, depth, sem = net._render_fn()(net, o, d, nrm, aabb, T, t, None, u, 0.2)
        (image.sum() + depth.sum() + sem.sum()).backward()
        for p in net.parameters():
            p.grad = None
        traces.append(rec.take())
    return traces


def run_infer(net, rec, settings):
    fresh(net, **settings).eval()
    o, d, nrm, aabb, u = _rays(N_INFER, T)
    traces = []
    for _ in range(2):
        with torch.no_grad():
            net._run_infer(o, d, nrm, aabb, T, T, None, u, 0.2)
        traces.append(rec.take())
    return traces


def run_case(net, rec, case):
    if case.startswith("train/"):
        return run_train(net, rec, *train_cases()[case])
    return run_infer(net, rec, infer_cases()[case])


ALL_CASES = list(train_cases()) + list(infer_cases())


@functools.lru_cache(maxsize=None)
def _golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


def test_the_fixture_holds_exactly_these_cases():
    assert len(train_cases()) == 44 + 4 and len(infer_cases()) == 10
    assert sorted(_golden()["cases"]) == sorted(ALL_CASES)


@pytest.mark.parametrize("case", ALL_CASES)
def test_trace_equals_the_recorded_one(case, monkeypatch):
    net = _net()
    rec = install(monkeypatch, net)
    got = run_case(net, rec, case)
    g = _golden()
    want = [[g["calls"][c] for c in g["traces"][i]] for i in g["cases"][case]]
    assert len(got) == len(want)
    for step, (a, b) in enumerate(zip(got, want)):
        assert a == b, (case, step)
    # the cache itself, said once more in words
    packs = [[ln for ln in tr if is_pack(ln)] for tr in got]
    assert packs[0] and packs[1] == []
    assert all("out=none" in ln for ln in packs[0])
    if case.startswith("train/"):
        # an update: every form the mode uses is packed again, into its old buffer
        # (a pack made from a rounded COPY of the parameters never had one)
        assert packs[2] == [ln if "params=copy" in ln else ln.replace("out=none", "out=given")
                            for ln in packs[0]]


def test_precision_errors(monkeypatch):
    net = _net()
    rec = install(monkeypatch, net)
    o, d, nrm, aabb, u = _rays(N_INFER, T)
    with torch.no_grad():
        fresh(net, precision="fp8")
        with pytest.raises(ValueError, match="precision must be fp32, bf16x3, f16x2 or fp16, got fp8"):
            net._run_infer(o, d, nrm, aabb, T, T, None, u, 0.2)
        fresh(net, precision="bf16x3", fp16_table=True)
        with pytest.raises(ValueError, match="fp16_table needs precision='fp16'"):
            net._run_infer(o, d, nrm, aabb, T, T, None, u, 0.2)
    assert rec.take() == []


# The marcher's selection (run_cuda refuses CPU tensors, so its helper is asked
# directly): precision, fused -> field, sigma-MLP op and pack, shade_mode, shade nets
SIGMA_PACK_ARG = {"sigma_mlp_fwd": "packed_sigma", "sigma_mlp_fwd_f16": "packed_sigma_half",
                  "sigma_mlp_fwd_x3": "packed_sigma_x3", "sigma_mlp_fwd_h2": "packed_sigma_h2"}
MARCH = [
    ("fp32", True, "mlp_pack", "sigma_mlp_fwd", "mlp_pack", False, "mlp_pack"),
    ("fp32", False, "mlp_pack", "sigma_mlp_fwd", "mlp_pack", False, "mlp_pack"),
    ("fp16", True, "mlp_pack_f16", "sigma_mlp_fwd_f16", "mlp_pack_f16", True, "mlp_pack_f16"),
    ("fp16", False, "mlp_pack", "sigma_mlp_fwd", "mlp_pack", False, "mlp_pack"),
    ("bf16x3", True, "mlp_pack", "sigma_mlp_fwd_x3", "mlp_pack_x3", False, "mlp_pack"),
    ("bf16x3", False, "mlp_pack", "sigma_mlp_fwd_x3", "mlp_pack_x3", False, "mlp_pack"),
    ("f16x2", True, "mlp_pack", "sigma_mlp_fwd_h2", "mlp_pack_h2", "f16x2", "mlp_pack_h2"),
    ("f16x2", False, "mlp_pack", "sigma_mlp_fwd_h2", "mlp_pack_h2", False, "mlp_pack"),
]


@pytest.mark.parametrize("precision,fused,field,sigma_op,sigma_pack,shade_mode,shade", MARCH)
def test_marcher_selection(precision, fused, field, sigma_op, sigma_pack, shade_mode, shade,
                           monkeypatch):
    net = _net()
    rec = install(monkeypatch, net)
    fresh(net, precision=precision).eval()
    with torch.no_grad():
        f, sigma_mlp, mode, nets = net._march_arith(fused)
        rec.take()
        sigma_mlp(torch.zeros(16, 3, 2))
    assert [f[k]._tag for k in ("packed_sigma", "packed_color", "packed_sem")] == \
        [f"{field}:{n}" for n in ("sigma", "color", "sem")]
    assert rec.label(f["table"]) == "param:grid" and f["grid"] is net.encoder.grid
    assert rec.take() == [f"{sigma_op} {SIGMA_PACK_ARG[sigma_op]}={sigma_pack}:sigma"]
    assert type(mode) is type(shade_mode) and mode == shade_mode
    assert [nets[k]._tag for k in ("packed_color", "packed_sem")] == [f"{shade}:color", f"{shade}:sem"]




def test_marcher_selection_rejects_an_unknown_precision(monkeypatch):
    net = _net()
    install(monkeypatch, net)
    fresh(net, precision="fp8")
    with pytest.raises(ValueError, match="precision must be fp32, bf16x3, f16x2 or fp16, got fp8"):
        net._march_arith(True)


def record():
    """Write the fixture from the tree this file sits in."""
    net = _net()
    calls, traces, cases = {}, {}, {}
    with pytest.MonkeyPatch.context() as mp:
        rec = install(mp, net)
        for case in ALL_CASES:
            ids = []
            for tr in run_case(net, rec, case):
                key = tuple(calls.setdefault(ln, len(calls)) for ln in tr)
                ids.append(traces.setdefault(key, len(traces)))
            cases[case] = ids
    def rows(items):       # one call, trace or case per line
        return ",\n".join(json.dumps(i, separators=(",", ":")) for i in items)
    with open(GOLDEN, "w") as fh:
        fh.write('{"calls":[\n' + rows(calls) + '],\n"traces":[\n' + rows(list(k) for k in traces)
                 + '],\n"cases":{\n' + ",\n".join(f"{json.dumps(c)}:{json.dumps(cases[c], separators=(',', ':'))}"
                                                  for c in sorted(cases)) + "}}\n")
    print(f"{len(cases)} cases, {len(traces)} distinct traces, {len(calls)} distinct calls, "
          f"{sum(len(k) for k in traces)} calls in them")


if __name__ == "__main__":
    record()
