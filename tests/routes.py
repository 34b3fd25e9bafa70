"""Which entry point does a projection call take?  The bit-equality contracts of include/ivl_hip.h make every route of the dispatch
ladder give the same numbers, so a call that falls to the library GEMM by mistake is only slower: no comparison of
outputs sees it.  This helper records the route itself.

`record()` puts a proxy in place of the loaded library that notes the name of every `ivl_*` function called, runs a fixed grid of
eager calls through ops.linear / linear_swiglu / linear_m16 / linear_m64 / gdn_out_linear, and returns {case: [symbols in call
order]}; a case in which no projection symbol ran starts with "library", one that raised ends with "raise <type>".

tests/routes_expected.json is this grid recorded ONCE on the commit before the dispatch was rewritten as one ladder (7fbcec5):
    python tests/routes.py --write
tests/test_gpu_routes.py compares the grid on the current code with it, case by case.  A new route changes the file on purpose, in
the pull request that adds the route."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
EXPECTED = os.path.join(HERE, "routes_expected.json")
DEV = "cuda:0"
BF = torch.bfloat16
N = 48                                   # output columns (GLU: I); the one m256 case has I = 6148
ROWS = (1, 4, 5, 16, 17, 33, 64, 65)     # both sides of every border of the ladder: 4 | 5, 16 | 17, wide_rows 32 | 33, 64 | 65
FMTS = ("bf16", "e4m3", "mxfp4")
WIDE = {"off": {}, "16": {"wide": True}, "32": {"wide": True, "wide_rows": 32}, "64": {"wide": True, "wide_rows": 64}}
# the adapter settings per wide setting: no table, a table, a table with wide_lora, the same with ops._LORA_FUSED on
LORA = {"off": ("none", "table"), "16": ("none", "table", "wide_lora", "wide_lora+fused"), "32": ("none", "wide_lora"),
        "64": ("none", "wide_lora")}


class _Recorder:
    """the loaded library, every ivl_* call noted by name"""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("ivl_") or name == "ivl_last_error":
            return fn

        def call(*args):
            self._log.append(name)
            return fn(*args)
        return call


def _weights(K, R, fmt, gen):
    from infinitevl_amd import ops
    w = (torch.randn(R, K, generator=gen) * K ** -0.5).to(BF).to(DEV)
    return w, (None if fmt == "bf16" else ops.PackedWeight.of(w, fmt=fmt))


def _table(R, K, glu, gen):
    """a rank-8 table with one adapter over the projection "p" (GLU: the two segments gate | up)"""
    from infinitevl_amd import ops
    t = ops.LoraTable(2, 8, DEV)
    borders = (0, R // 2, R) if glu else (0, R)
    t.register("p", R, K, borders)
    t.load({"p": [((torch.randn(8, K, generator=gen) * 0.1).to(BF), (torch.randn(b - a, 8, generator=gen) * 0.1).to(BF))
                  for a, b in zip(borders, borders[1:])]}, 0.5)
    return t


def _input(rows, K, kind, gen):
    from infinitevl_amd import ops
    x = torch.randn(rows, K, generator=gen).to(BF).to(DEV)
    if kind == "prenorm":
        return ops.PreNorm(x, torch.randn(rows, K, generator=gen).to(BF).to(DEV), torch.ones(K, dtype=BF, device=DEV), 1e-5)
    if kind == "strided":                # the K columns of a wider buffer: not contiguous from two rows on
        return torch.randn(rows, 2 * K, generator=gen).to(BF).to(DEV)[:, :K]
    return x


def _cases():
    """(name, thunk) of every call of the grid; a thunk takes nothing and makes the one call"""
    from infinitevl_amd import ops
    import projections as pj
    gen = torch.Generator().manual_seed(7)
    out = []

    def ladder(name, glu, w, pw, bias, rows, K, kind, wide, lora, table):
        def run():
            x = _input(rows, K, kind, gen)
            kw = dict(WIDE[wide])
            if pw is not None:
                kw["w8"] = pw
            if lora != "none":
                idx = torch.tensor([0, -1] * rows, dtype=torch.int32)[:rows].to(DEV)          # every other row has the adapter
                kw["lora"] = (table, "p", idx)
                if lora.startswith("wide_lora"):
                    kw["wide_lora"] = True
            was, ops._LORA_FUSED = ops._LORA_FUSED, lora.endswith("fused")
            try:
                return ops.linear_swiglu(x, w, **kw) if glu else ops.linear(x, w, bias, **kw)
            finally:
                ops._LORA_FUSED = was
        out.append((name, run))

    for glu in (False, True):
        form = "glu" if glu else "plain"
        for K in (64, 512):
            for fmt in FMTS:
                w, pw = _weights(K, 2 * N if glu else N, fmt, gen)
                bias = None if glu else torch.randn(N, generator=gen).to(BF).to(DEV)
                table = _table(w.shape[0], K, glu, gen)
                # K = 512 is there for the fused norm launch (512 <= K <= 4096): with a tensor input it repeats K = 64
                for kind, rows_of in (("tensor", ROWS if K == 64 else ()), ("prenorm", (1, 4, 5, 16, 17))):
                    for rows in rows_of:
                        for wide, loras in LORA.items():
                            for lora in loras:
                                ladder(f"{form} {fmt} K={K} rows={rows} x={kind} wide={wide} lora={lora}", glu, w, pw, bias, rows, K,
                                       kind, wide, lora, table)
                if K == 64 and glu:      # a prefill chunk's row count at a narrow I: the m256 kernel does not apply
                    for wide in ("off", "64"):
                        ladder(f"glu {fmt} K=64 rows=256 x=tensor wide={wide} lora=none", True, w, pw, None, 256, 64, "tensor", wide,
                               "none", None)
                if K == 64:              # the direct entries: no row check in Python, the ABI's refusal raises
                    for fn, tag in ((ops.linear_m16, "m16"), (ops.linear_m64, "m64")):
                        for rows in (1, 16, 17, 64, 65):
                            out.append((f"direct {tag} {form} {fmt} rows={rows}",
                                        lambda fn=fn, rows=rows, w=w, pw=pw, bias=bias, glu=glu:
                                        fn(_input(rows, 64, "tensor", gen), w, bias, glu=glu, w8=pw)))
    # the one shape the 256-row kernel takes (6144 < I <= 12288), in front of the wide routes
    w256, _ = _weights(64, 2 * 6148, "bf16", gen)
    for wide in ("off", "64"):
        ladder(f"glu bf16 K=64 I=6148 rows=256 x=tensor wide={wide} lora=none", True, w256, None, None, 256, 64, "tensor", wide, "none", None)
    # calls that a predicate turns away: x not contiguous, a bias that is not bf16, K no multiple of 32
    w, _ = _weights(64, N, "bf16", gen)
    wg, _ = _weights(64, 2 * N, "bf16", gen)
    w48, _ = _weights(48, N, "bf16", gen)
    wg48, _ = _weights(48, 2 * N, "bf16", gen)
    b32 = torch.randn(N, generator=gen).to(DEV)
    for rows in (4, 5, 17):
        ladder(f"plain bf16 K=64 rows={rows} x=strided wide=64 lora=none", False, w, None, None, rows, 64, "strided", "64", "none", None)
        ladder(f"glu bf16 K=64 rows={rows} x=strided wide=64 lora=none", True, wg, None, None, rows, 64, "strided", "64", "none", None)
        ladder(f"plain bf16 K=64 rows={rows} x=tensor bias=fp32 wide=64 lora=none", False, w, None, b32, rows, 64, "tensor", "64", "none", None)
        ladder(f"plain bf16 K=48 rows={rows} x=tensor wide=64 lora=none", False, w48, None, None, rows, 48, "tensor", "64", "none", None)
        ladder(f"glu bf16 K=48 rows={rows} x=tensor wide=64 lora=none", True, wg48, None, None, rows, 48, "tensor", "64", "none", None)
    # the decode step's o_proj behind the gated norm
    c = pj.gdn_out_case(2, N)
    for fmt in FMTS:
        wo = c["w"].to(DEV)
        pw = None if fmt == "bf16" else ops.PackedWeight.of(wo, fmt=fmt)
        for M in (1, 4):
            def run(wo=wo, pw=pw, M=M):
                dev = lambda t: t[:M].to(DEV)      # noqa: E731
                return ops.gdn_out_linear(dev(c["o_raw"]).view(M, 1, -1), dev(c["proj"]).view(M, 1, c["ld"]), c["col_g"], c["col_q"],
                                          c["col_k"], c["nw"].to(DEV), c["eps"], dev(c["cq"]), dev(c["ck"]), wo, c["bias"].to(DEV),
                                          c["H"], w8=pw)
            out.append((f"gdn_out {fmt} rows={M}", run))
    return out


def record():
    """{case: [symbols]} of the whole grid on the code at hand"""
    from infinitevl_amd import _lib
    real = _lib.load()
    cases = _cases()
    log, routes = [], {}
    _lib._lib = _Recorder(real, log)
    try:
        for name, run in cases:
            del log[:]
            tail = []
            try:
                run()
            except Exception as e:       # noqa: BLE001 -- a refusal is a route too
                tail = [f"raise {type(e).__name__}"]
            assert name not in routes, name
            routes[name] = ([] if any("linear" in s for s in log) else ["library"]) + list(log) + tail
        torch.cuda.synchronize()
    finally:
        _lib._lib = real
    return routes


def expected():
    with open(EXPECTED) as f:
        return json.load(f)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(HERE))
    got = record()
    if "--write" in sys.argv[1:]:        # --write [PATH]
        path = (sys.argv[sys.argv.index("--write") + 1:] + [EXPECTED])[0]
        with open(path, "w") as f:
            f.write("{\n" + ",\n".join(f"{json.dumps(k)}: {json.dumps(v)}" for k, v in got.items()) + "\n}\n")
        print(f"{len(got)} cases written to {path}")
    else:
        want = expected()
        bad = [k for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)]
        for k in bad:
            print(f"{k}: expected {want.get(k)}, got {got.get(k)}")
        print(f"{len(got)} cases, {len(bad)} differ")
        sys.exit(1 if bad else 0)
