"""Record what the weight-gradient planner (plan_wgrad, csrc/vq2_wgrad.hip) decides for a list of layer shapes, into
tests/golden/wgrad_plans.json.  tests/test_host_cpu.py::test_wgrad_plans_match_the_recorded_ones replays the file.

What is recorded is what the library shows of a plan without launching anything (no GPU needed): the workspace size
(vq2_conv_wgrad_workspace_bytes) and the fields of the reduction job (vq2_wgrad_job_init) -- O, I, Or, Ir, taps, S,
n_units_w, n_units_b, swapped (bit 0 exchanged roles, bits 1-2 the Winograd mode), bias_splits -- each with and without a bias gradient, under VQ2_FORMS = all, direct and
general.  The library reads VQ2_FORMS once per process: `all` is recorded in this process, the other two in a child each
(`--replay FILE` is that child: it prints the plans of the shapes in FILE under the VQ2_FORMS it was started with).

The shapes:
  * stage 1: every conv spec of VQVAE and VQVAE_Deep at the resolutions of the bench.py workloads (c2 / deep: batch 32 from
    256x256 down to 32x32; c5: batch 8 from 512x512 down to 64x64);
  * stage 2: every conv spec of the top (32x32, batch 32) and bottom (64x64 and its 32x32 condition, batch 8) PixelSNAIL;
  * the wgrad rows of CASES (tests/test_gpu_dispatch.py) and GEOM_CASES (tests/test_gpu_geom_dispatch.py), with dense
    operands and with the 8-channel wider buffers those tests use;
  * BOUNDARIES below: one step either side of every condition of plan_wgrad.

THE FILE IS A RECORDING, NOT A SPECIFICATION: it holds what the planner decided at the commit that wrote it, so that a
refactor of the planner can show that it decided nothing anew.  A change that moves a plan on purpose runs this script
again, commits the new file and says which entries moved (git diff of the JSON shows them, one line per entry)."""
import argparse
import ctypes
import importlib.util
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "wgrad_plans.json")
FIELDS = ["ws_bytes", "O", "I", "Or", "Ir", "taps", "S", "n_units_w", "n_units_b", "swapped", "bias_splits"]
FORMS = ("all", "direct", "general")
# The two layouts of an entry's integer list, by its "kind" (the file predates the one descriptor and keeps them): the
# first form of vq2_conv_desc with its one `pad`, and the same_size form, which states neither stride nor transposed
DESC = ("N", "H", "W", "Ci", "Co", "KH", "KW", "stride", "pad", "transposed", "ldx", "ldy", "Cir", "Cor")
GEOM = ("N", "H", "W", "Ci", "Co", "KH", "KW", "pad_top", "pad_left", "ldx", "ldy", "Cir", "Cor")


def descriptor(L, e):
    """vq2_conv_desc of an entry."""
    d = L.ConvDesc()
    if e["kind"] == "geom":
        v = dict(zip(GEOM, e["d"]), stride=1, transposed=0, same_size=1)
    else:
        v = dict(zip(DESC, e["d"]), same_size=0)
        v["pad_top"] = v["pad_left"] = v.pop("pad")
    for n, x in v.items():
        setattr(d, n, x)
    return d


def load_binding():
    """The ctypes binding alone (vqvae2_amd/_lib.py by path): the package's ops.py is not needed to plan."""
    spec = importlib.util.spec_from_file_location("vq2_lib", os.path.join(ROOT, "vq-vae-2-pytorch_amd", "_lib.py"))
    L = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(L)
    return L


def plans(entries, L):
    """[[fields with db], [fields without db]] for every entry ({"kind": "desc" | "geom", "d": [descriptor ints]}) under
    the VQ2_FORMS of this process.  job_init gets non-null 16-byte aligned addresses of a real host allocation."""
    backing = ctypes.create_string_buffer(4096 + 16)
    ptr = ctypes.c_void_p((ctypes.addressof(backing) + 15) & ~15)
    out = []
    for e in entries:
        d = descriptor(L, e)
        both = []
        for db in (ptr, None):
            job = L.WgradJob()
            rc = L.lib.vq2_wgrad_job_init(ctypes.byref(d), ptr, ptr, db, ctypes.byref(job))
            if rc != 0:
                raise RuntimeError("%s: %s" % (e, L.lib.vq2_last_error().decode()))
            both.append([int(L.lib.vq2_conv_wgrad_workspace_bytes(ctypes.byref(d)))] + [int(getattr(job, f)) for f in FIELDS[1:]])
        out.append(both)
    return out


def ceil4(c):
    return (c + 3) // 4 * 4


def desc(src, tr, cin, cout, k, stride, pad, n, h, w, wider=0):
    ci, co = ceil4(cin), ceil4(cout)
    return {"src": src, "kind": "desc", "d": [n, h, w, ci, co, k, k, stride, pad, int(tr), ci + wider, co + wider, cin, cout]}


def geom(src, cin, cout, g, n, h, w, wider=0):
    ci, co = ceil4(cin), ceil4(cout)
    return {"src": src, "kind": "geom", "d": [n, h, w, ci, co, g[0], g[1], g[2], g[3], ci + wider, co + wider, cin, cout]}


def of_spec(src, s, n, h, w):
    if s.same_size:
        return geom(src, s.cin, s.cout, (s.k, s.kw, s.pad_top, s.pad_left), n, h, w)
    return desc(src, s.transposed, s.cin, s.cout, s.k, s.stride, s.pad, n, h, w)


def model_specs(model):
    from vqvae2_amd.ops import ConvSpec
    seen = []
    for mod in model.modules():
        for v in vars(mod).values():
            for s in (v if isinstance(v, (list, tuple)) else (v,)):
                if isinstance(s, ConvSpec) and s not in seen:
                    seen.append(s)
    return seen


F, T = False, True
BOUNDARIES = [
    # transposed, cin, cout, k, stride, pad, N, H, W
    # exchanged roles: Co 32 | 36, Ci 60 | 64, centred square kernels only, not 1x1
    (F, 64, 32, 3, 1, 1, 4, 3, 32), (F, 64, 36, 3, 1, 1, 4, 3, 32), (F, 60, 32, 3, 1, 1, 4, 3, 32), (F, 128, 32, 3, 1, 1, 4, 3, 32),
    (F, 64, 32, 5, 1, 2, 4, 3, 32), (F, 64, 32, 3, 1, 0, 4, 5, 34), (F, 64, 32, 1, 1, 0, 4, 3, 32), (F, 64, 28, 3, 1, 1, 4, 3, 32),
    # the 128 x 96 tile (K = 288): M 65535 | 65536, plain and exchanged
    (F, 32, 128, 3, 1, 1, 15, 17, 257), (F, 32, 128, 3, 1, 1, 2048, 1, 32), (F, 128, 32, 3, 1, 1, 15, 17, 257), (F, 128, 32, 3, 1, 1, 2048, 1, 32),
    (F, 32, 128, 3, 1, 1, 1, 256, 256), (F, 128, 32, 3, 1, 1, 1, 256, 256),
    # Winograd mode 1 (3x3 128 -> 128) and mode 3 (128 -> 32): W 32 / 40 / 64, H odd / even
    (F, 128, 128, 3, 1, 1, 4, 3, 32), (F, 128, 128, 3, 1, 1, 4, 4, 32), (F, 128, 128, 3, 1, 1, 4, 3, 40), (F, 128, 128, 3, 1, 1, 4, 4, 40),
    (F, 128, 128, 3, 1, 1, 4, 3, 64), (F, 128, 128, 3, 1, 1, 4, 4, 64), (F, 128, 128, 3, 1, 1, 4, 4, 96), (F, 128, 128, 3, 1, 1, 4, 4, 128),
    (F, 128, 32, 3, 1, 1, 4, 4, 32), (F, 128, 32, 3, 1, 1, 4, 3, 40), (F, 128, 32, 3, 1, 1, 4, 4, 40), (F, 128, 32, 3, 1, 1, 4, 3, 64),
    (F, 128, 32, 3, 1, 1, 4, 4, 64), (F, 256, 32, 3, 1, 1, 4, 4, 64), (F, 132, 32, 3, 1, 1, 4, 4, 64), (F, 128, 28, 3, 1, 1, 4, 4, 64),
    # O, I at 124 / 128 / 132 (mode 1)
    (F, 124, 128, 3, 1, 1, 4, 4, 64), (F, 132, 128, 3, 1, 1, 4, 4, 64), (F, 128, 124, 3, 1, 1, 4, 4, 64), (F, 128, 132, 3, 1, 1, 4, 4, 64),
    (F, 124, 124, 3, 1, 1, 4, 4, 64), (F, 132, 132, 3, 1, 1, 4, 4, 64), (F, 256, 256, 3, 1, 1, 4, 4, 64), (F, 128, 256, 3, 1, 1, 4, 4, 64),
    # mode 2, 4x4 stride 2: width of the G grid 32 / 40 / 64, its height odd / even, I == 64 | 60 | 68 | 128 | 132, O 124 / 128 / 132
    (F, 64, 128, 4, 2, 1, 4, 6, 64), (F, 64, 128, 4, 2, 1, 4, 8, 64), (F, 64, 128, 4, 2, 1, 4, 6, 80), (F, 64, 128, 4, 2, 1, 4, 8, 80),
    (F, 64, 128, 4, 2, 1, 4, 6, 128), (F, 64, 128, 4, 2, 1, 4, 8, 128), (F, 60, 128, 4, 2, 1, 4, 8, 128), (F, 68, 128, 4, 2, 1, 4, 8, 128),
    (F, 128, 128, 4, 2, 1, 4, 8, 128), (F, 132, 128, 4, 2, 1, 4, 8, 128), (F, 64, 124, 4, 2, 1, 4, 8, 128), (F, 64, 132, 4, 2, 1, 4, 8, 128),
    (F, 32, 128, 4, 2, 1, 4, 8, 128), (F, 64, 256, 4, 2, 1, 4, 8, 128),
    # ... and the conv-transpose of the pair (roles exchanged by the layer: O = Ci, I = Co)
    (T, 128, 64, 4, 2, 1, 4, 3, 32), (T, 128, 64, 4, 2, 1, 4, 4, 32), (T, 128, 64, 4, 2, 1, 4, 3, 40), (T, 128, 64, 4, 2, 1, 4, 3, 64),
    (T, 128, 64, 4, 2, 1, 4, 4, 64), (T, 128, 60, 4, 2, 1, 4, 4, 64), (T, 128, 68, 4, 2, 1, 4, 4, 64), (T, 128, 128, 4, 2, 1, 4, 4, 64),
    (T, 124, 64, 4, 2, 1, 4, 4, 64), (T, 132, 64, 4, 2, 1, 4, 4, 64), (T, 64, 3, 4, 2, 1, 4, 4, 64), (T, 64, 64, 4, 2, 1, 4, 4, 64),
    (T, 128, 64, 4, 2, 1, 32, 64, 64), (F, 64, 128, 4, 2, 1, 32, 128, 128),
    # the reach of the Winograd modes: 2^29 elements of x or dy over the input grid (x 4 for conv-transpose), one image either side
    (F, 128, 128, 3, 1, 1, 1023, 64, 64), (F, 128, 128, 3, 1, 1, 1024, 64, 64), (F, 128, 32, 3, 1, 1, 1023, 64, 64),
    (F, 128, 32, 3, 1, 1, 1024, 64, 64), (T, 128, 64, 4, 2, 1, 511, 64, 64), (T, 128, 64, 4, 2, 1, 512, 64, 64),
    (F, 64, 128, 4, 2, 1, 511, 128, 128), (F, 64, 128, 4, 2, 1, 512, 128, 128),
    # S: 1 (M <= 256), max_s = ceil(M / 256) on either side of a multiple of 256, the resident slots (S well above 32)
    (F, 64, 64, 1, 1, 0, 1, 2, 32), (F, 64, 64, 1, 1, 0, 1, 8, 32), (F, 64, 64, 1, 1, 0, 1, 8, 33), (F, 64, 64, 1, 1, 0, 3, 8, 32),
    (F, 64, 64, 1, 1, 0, 32, 64, 64), (F, 64, 64, 1, 1, 0, 32, 63, 65), (F, 128, 128, 3, 1, 1, 32, 16, 16), (F, 128, 128, 3, 1, 1, 33, 31, 33),
    (F, 256, 256, 1, 1, 0, 32, 32, 32), (F, 3, 64, 4, 2, 1, 32, 256, 256), (F, 16, 40, 7, 1, 3, 32, 32, 32), (F, 512, 512, 3, 1, 1, 8, 16, 16),
]


def shapes():
    """Every entry to record: {"src", "kind", "d"} (see plans)."""
    sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
    import vqvae2_amd as A
    import test_gpu_dispatch as D
    import test_gpu_geom_dispatch as G
    out = []
    for name, model, sizes in (("vqvae", A.VQVAE(), ((32, 256), (8, 512))), ("vqvae_deep", A.VQVAE_Deep(), ((32, 256),))):
        for s in model_specs(model):
            for n, size in sizes:
                for level in range(4):
                    out.append(of_spec(name, s, n, size >> level, size >> level))
    top = A.PixelSNAIL([32, 32], 512, 256, 5, 4, 4, 256)
    bottom = A.PixelSNAIL([64, 64], 512, 256, 5, 4, 4, 256, attention=False, n_cond_res_block=3, cond_res_channel=256)
    out += [of_spec("pixelsnail_top", s, 32, 32, 32) for s in model_specs(top)]
    out += [of_spec("pixelsnail_bottom", s, 8, hw, hw) for s in model_specs(bottom) for hw in (64, 32)]
    for c in D.CASES:
        if c[0] == "wgrad":
            out += [desc("CASES", *c[1:10], wider=wider) for wider in (0, 8)]
    for c in G.GEOM_CASES:
        if c[0] == "wgrad":
            out += [geom("GEOM_CASES", *c[1:7], wider=wider) for wider in (0, 8)]
    out += [desc("boundary", *b) for b in BOUNDARIES]
    uniq, seen = [], set()
    for e in out:   # a shape that two sources name is recorded once, under the first
        key = (e["kind"], tuple(e["d"]))
        if key not in seen:
            seen.add(key)
            uniq.append(e)
    return uniq


def replay_in_child(forms, path):
    env = dict(os.environ, VQ2_FORMS=forms)
    return subprocess.Popen([sys.executable, os.path.abspath(__file__), "--replay", path], env=env, stdout=subprocess.PIPE,
                            stderr=subprocess.PIPE, text=True)


def child_result(proc):
    out, err = proc.communicate(timeout=600)
    if proc.returncode != 0:
        raise RuntimeError(err[-2000:])
    return json.loads(out.strip().splitlines()[-1])


def write(path, entries):
    with open(path, "w") as f:   # one line per entry: a plan that moves shows as one changed line
        f.write('{"fields": %s,\n "entries": [\n' % json.dumps(FIELDS))
        f.write(",\n".join("  " + json.dumps(e) for e in entries))
        f.write("\n ]}\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--replay", metavar="FILE", help="print the plans of FILE's shapes under this process's VQ2_FORMS")
    ap.add_argument("--out", default=GOLDEN)
    args = ap.parse_args()
    if args.replay:
        with open(args.replay) as f:
            print(json.dumps(plans(json.load(f)["entries"], load_binding())))
        return
    if os.environ.get("VQ2_FORMS", "all") != "all":
        raise SystemExit("record with VQ2_FORMS unset: this process records `all`, children the other two")
    entries = shapes()
    write(args.out, entries)                       # the children read the shapes from the file
    kids = {forms: replay_in_child(forms, args.out) for forms in FORMS[1:]}
    got = {"all": plans(entries, load_binding())}
    got.update({forms: child_result(p) for forms, p in kids.items()})
    for i, e in enumerate(entries):
        for forms in FORMS:
            e[forms] = got[forms][i]
    write(args.out, entries)
    print("wrote %s: %d shapes x %d forms x (with, without db)" % (args.out, len(entries), len(FORMS)))


if __name__ == "__main__":
    main()
