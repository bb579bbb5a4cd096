"""CPU-side checks: the C-ABI library loads and exports every symbol include/vq2.h declares (no
compute calls without a GPU), host logic (module layout, fusion plan, scheduler) behaves."""
import ctypes
import os
import re

import pytest
import torch

from oracle import vqvae_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def amd():
    import vqvae2_amd
    return vqvae2_amd


def test_library_exports_every_declared_symbol(amd):
    hdr = open(os.path.join(ROOT, "include", "vq2.h")).read()
    declared = set(re.findall(r"\b(vq2_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 25
    lib = ctypes.CDLL(amd._lib.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in vq2.h but not exported"
    assert declared == set(amd._lib.EXPORTS), declared ^ set(amd._lib.EXPORTS)
    assert lib.vq2_version() == amd._lib.API_VERSION == int(re.search(r"#define\s+VQ2_API_VERSION\s+(\d+)", hdr).group(1))


def test_conv_desc_binding_matches_the_header(amd):
    """The ctypes mirror of vq2_conv_desc: sixteen int32 words, 64 bytes without padding, in the header's order."""
    hdr = open(os.path.join(ROOT, "include", "vq2.h")).read()
    body = re.search(r"typedef struct vq2_conv_desc \{(.*?)\} vq2_conv_desc;", hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [s.strip() for s in body.split(";") if s.strip()]
    assert all(s.startswith("int32_t ") for s in decls), decls
    names = [n.strip() for s in decls for n in s[len("int32_t "):].split(",")]
    D = amd._lib.ConvDesc
    assert [n for n, _ in D._fields_] == names and len(names) == 16
    assert all(t is ctypes.c_int32 for _, t in D._fields_)
    assert ctypes.sizeof(D) == 64 and [getattr(D, n).offset for n in names] == list(range(0, 64, 4))


def test_hot_kernels_do_not_spill():
    """The compiler's resource report written by csrc/build.sh: none of the kernels the train step runs may spill a
    register or use scratch memory (round 2: ONE spilled VGPR in the four-per-CU conv tile = 3 % of the whole step,
    invisible to every functional test)."""
    import glob
    files = glob.glob(os.path.join(ROOT, "vq-vae-2-pytorch_amd", "csrc", "_obj", "*.res"))
    if not files:
        pytest.skip("no resource reports: run __graft_entry__.build() first")
    hot = re.compile(r"conv_gemm_fast_kernel|wino3_kernel|wino_k4s2_kernel|wino_subpixel_kernel|rbw_fwd_kernel|conv1x1_k64_kernel|wgrad_fast_kernel|resblock_|subpixel_conv|vq_fwd_kernel|conv_k4s2_c4|"
                     r"convT_small_mfma|vq_stats_|wgrad_reduce_batched|adam_kernel|mse_")
    seen = 0
    for f in files:
        name = None
        for line in open(f):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
                seen += bool(hot.search(name))
                continue
            m = re.search(r"(VGPRs Spill|SGPRs Spill|ScratchSize \[bytes/lane\]): (\d+)", line)
            if m and name and hot.search(name):
                assert int(m.group(2)) == 0 or m.group(1) == "SGPRs Spill" and int(m.group(2)) <= 16, \
                    f"{name}: {m.group(1)} = {m.group(2)}"
    assert seen >= 40, f"only {seen} hot kernels found in the reports"


def test_weight_gradient_plans_and_slab_layouts_without_gpu(amd):
    """Host side of the weight-gradient launches (pure planning code, no device): which shapes take the Winograd-domain
    kernels, how large their slab workspaces are, and what the reduction job says about the slab layout
    (vq2_wgrad_job.swapped: bit 0 exchanged roles, bits 1-2 the Winograd mode)."""
    lib = amd._lib.lib
    lib.vq2_conv_wgrad_workspace_bytes.restype = ctypes.c_size_t

    def plan(cin, cout, k, stride, pad, transposed, n, h, w):
        d = amd._lib.ConvDesc()
        d.N, d.H, d.W, d.Ci, d.Co, d.KH, d.KW, d.stride, d.pad_top, d.pad_left = n, h, w, cin, cout, k, k, stride, pad, pad
        d.transposed, d.ldx, d.ldy, d.Cir, d.Cor = int(transposed), cin, cout, cin, cout
        job = amd._lib.WgradJob()
        dummy = ctypes.c_void_p(16)
        rc = lib.vq2_wgrad_job_init(ctypes.byref(d), dummy, dummy, dummy, ctypes.byref(job))
        assert rc == 0, lib.vq2_last_error()
        return lib.vq2_conv_wgrad_workspace_bytes(ctypes.byref(d)), job

    # 3x3 128 -> 128 at 64x64: F(2,3) over column pairs -- K axis 12 * I, one thread column per (o, kh, i) in the reduction
    ws, job = plan(128, 128, 3, 1, 1, False, 32, 64, 64)
    assert (job.swapped >> 1) & 3 == 1 and job.swapped & 1 == 0 and job.taps == 9
    assert job.n_units_w == 128 * 3 * 128 // 32 and job.n_units_b == 128 // 32
    assert ws == (job.S * 128 * 12 * 128 + job.S * 128) * 4
    # the same layer at 32x32: rows of 16 pairs, two image rows per 32-pair chunk -- still the Winograd layout
    ws, job = plan(128, 128, 3, 1, 1, False, 32, 32, 32)
    assert (job.swapped >> 1) & 3 == 1 and ws == (job.S * 128 * 12 * 128 + job.S * 128) * 4
    # ... and at 16x16 (neither whole 64- nor 32-pixel rows): direct form, K axis 9 * I
    ws, job = plan(128, 128, 3, 1, 1, False, 32, 16, 16)
    assert job.swapped == 0 and job.n_units_w == 128 * 9 * 128 // 32 and ws == (job.S * 128 * 9 * 128 + job.S * 128) * 4
    # 4x4 stride-2 64 -> 128 from 128x128, and the conv-transpose 128 -> 64 to 128x128: F(2,2) by column parity, K axis 24 * I
    ws, job = plan(64, 128, 4, 2, 1, False, 32, 128, 128)
    assert (job.swapped >> 1) & 3 == 2 and job.n_units_w == 128 * 8 * 64 // 32 and job.bias_splits == 0
    assert ws == (job.S * 128 * 24 * 64 + job.S * 128) * 4
    ws, job = plan(128, 64, 4, 2, 1, True, 32, 64, 64)
    assert (job.swapped >> 1) & 3 == 2 and job.O == 128 and job.I == 64 and job.bias_splits == 4 * job.S
    assert ws == (job.S * 128 * 24 * 64 + job.S * 4 * 64) * 4
    # the ResBlock 3x3 (128 -> 32): exchanged roles + F(2,3), four 128 x 96 tiles (also at 32x32); direct exchanged roles at 16x16
    ws, job = plan(128, 32, 3, 1, 1, False, 32, 64, 64)
    assert job.swapped == 1 | (3 << 1) and job.O == 128 and job.I == 32 and job.n_units_w == 128 * 3 * 32 // 32
    assert ws == (job.S * 128 * 384 + job.S * 32) * 4
    ws, job = plan(128, 32, 3, 1, 1, False, 32, 32, 32)
    assert job.swapped == 1 | (3 << 1) and ws == (job.S * 128 * 384 + job.S * 32) * 4
    ws, job = plan(128, 32, 3, 1, 1, False, 32, 16, 16)
    assert job.swapped == 1 and ws == (job.S * 128 * 288 + job.S * 32) * 4
    # every plan keeps at least eight 32-row chunks per split and fills the resident slots
    for args in ((128, 128, 3, 1, 1, False, 32, 64, 64), (64, 128, 4, 2, 1, False, 32, 128, 128), (128, 32, 3, 1, 1, False, 8, 128, 128)):
        _, job = plan(*args)
        assert 1 <= job.S <= 256


_FORMS_CHILD = r"""
import ctypes, importlib.util, json, sys
spec = importlib.util.spec_from_file_location("vq2_lib", sys.argv[1])   # the binding alone: ops.py checks VQ2_FORMS too
L = importlib.util.module_from_spec(spec)
spec.loader.exec_module(L)
L.lib.vq2_conv_wgrad_workspace_bytes.restype = ctypes.c_size_t
out = {}
for cout in (128, 32):
    d = L.ConvDesc()
    d.N, d.H, d.W, d.Ci, d.Co, d.KH, d.KW, d.stride, d.pad_top, d.pad_left = 32, 64, 64, 128, cout, 3, 3, 1, 1, 1
    d.ldx, d.ldy, d.Cir, d.Cor = 128, cout, 128, cout
    job = L.WgradJob()
    dummy = ctypes.c_void_p(16)
    rc = L.lib.vq2_wgrad_job_init(ctypes.byref(d), dummy, dummy, dummy, ctypes.byref(job))
    out[cout] = dict(rc=rc, err=L.lib.vq2_last_error().decode(), swapped=job.swapped, S=job.S, n_units_w=job.n_units_w,
                     ws=L.lib.vq2_conv_wgrad_workspace_bytes(ctypes.byref(d)))
print(json.dumps(out))
"""


def test_forms_switch_plans_in_a_child_process(amd):
    """VQ2_FORMS turns whole families of forms off (csrc/vq2_common.h).  The library reads it once per process, so each
    value gets a child: "direct" plans the direct weight-gradient layout where the Winograd one is the default, "general"
    also stops exchanging the roles of x and dy, and any other value is refused by the library and by the package."""
    import json
    import subprocess
    import sys

    def run(value):
        env = dict(os.environ, VQ2_FORMS=value)
        r = subprocess.run([sys.executable, "-c", _FORMS_CHILD, amd._lib.__file__], env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return {int(k): v for k, v in json.loads(r.stdout.strip().splitlines()[-1]).items()}

    full, wide = 128 * 9 * 128 // 32, 128 * 3 * 128 // 32   # reduction units of the direct and the F(2,3) layouts
    p = run("all")
    assert p[128]["rc"] == 0 and (p[128]["swapped"] >> 1) & 3 == 1 and p[128]["n_units_w"] == wide
    assert p[32]["swapped"] == 1 | (3 << 1)
    p = run("direct")
    assert p[128]["rc"] == 0 and p[128]["swapped"] == 0 and p[128]["n_units_w"] == full
    assert p[128]["ws"] == (p[128]["S"] * 128 * 9 * 128 + p[128]["S"] * 128) * 4      # K axis 9 * I
    assert p[32]["rc"] == 0 and p[32]["swapped"] == 1                               # exchanged roles, direct form
    p = run("general")
    assert p[128]["swapped"] == 0 and p[128]["n_units_w"] == full
    assert p[32]["rc"] == 0 and p[32]["swapped"] == 0
    p = run("winograd")
    assert p[128]["rc"] != 0 and "VQ2_FORMS" in p[128]["err"] and p[128]["ws"] == 0
    r = subprocess.run([sys.executable, "-c", "import vqvae2_amd"], cwd=ROOT, env=dict(os.environ, VQ2_FORMS="winograd"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "VQ2_FORMS" in r.stderr, r.stderr[-2000:]


def test_wgrad_plans_match_the_recorded_ones(amd):
    """tests/golden/wgrad_plans.json (scripts/record_wgrad_plans.py) holds what plan_wgrad decided for every layer of the
    workloads, every weight-gradient row of the two dispatch tables and both sides of every plan condition, as far as the
    library shows it without a launch: workspace size and the reduction job, with and without a bias gradient, under every
    VQ2_FORMS.  Replayed here and compared exactly, this process's VQ2_FORMS in-process and the other values in a child each.
    The file is a recording of the commit that wrote it, not a specification: a change that moves a plan on purpose records
    it again and says which entries moved."""
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("record_wgrad_plans", os.path.join(ROOT, "scripts", "record_wgrad_plans.py"))
    rec = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(rec)
    with open(rec.GOLDEN) as f:
        golden = json.load(f)
    entries = golden["entries"]
    assert golden["fields"] == rec.FIELDS and len(entries) >= 300
    here = os.environ.get("VQ2_FORMS", "all")
    kids = {forms: rec.replay_in_child(forms, rec.GOLDEN) for forms in rec.FORMS if forms != here}
    got = {here: rec.plans(entries, amd._lib)}
    got.update({forms: rec.child_result(p) for forms, p in kids.items()})
    for forms in rec.FORMS:
        moved = [(e["src"], e["kind"], e["d"], e[forms], g) for e, g in zip(entries, got[forms]) if e[forms] != g]
        assert not moved, (forms, len(moved), moved[:3])
    # the recording reaches what it is there for: every role and Winograd mode, S = 1 and S > 32, both bias layouts
    modes = set(e["all"][0][rec.FIELDS.index("swapped")] for e in entries)
    assert modes == {0, 1, 2, 4, 7}, modes
    S = [e["all"][0][rec.FIELDS.index("S")] for e in entries]
    assert min(S) == 1 and max(S) > 32
    assert any(e["all"][0][-1] > 0 for e in entries) and any(e["all"][1][-3] == 0 < e["all"][0][-3] for e in entries)


def test_invalid_arguments_are_rejected_without_gpu(amd):
    lib = amd._lib.lib
    d = amd._lib.ConvDesc()
    assert lib.vq2_conv_fwd(ctypes.byref(d), 0, None, None, None, None, 0, None, None) == 1
    assert b"non-positive" in lib.vq2_last_error()
    d.N, d.H, d.W, d.Ci, d.Co, d.KH, d.KW, d.stride, d.pad_top, d.pad_left, d.ldx, d.ldy = 1, 8, 8, 6, 8, 3, 3, 1, 1, 1, 8, 8
    assert lib.vq2_conv_fwd(ctypes.byref(d), 0, None, None, None, None, 0, None, None) == 1
    assert b"multiples of 4" in lib.vq2_last_error()
    assert lib.vq2_vq_fwd(None, 0, None, None, None, 0, 0, 0, None, None, 0, None, None) == 1
    assert lib.vq2_vq_stats(None, 0, None, 0, 0, 0, None, None, None, 0, None) == 1
    assert lib.vq2_vq_stats_workspace_bytes(131072, 64, 8192) > 131072 * 8
    assert lib.vq2_adam_step(None, None, None, None, 0, 1e-3, .9, .999, 1e-8, 1, 1.0, None) == 1
    with pytest.raises(RuntimeError):
        amd._lib.check(1, "x")
    # tensors from 2^31 elements are refused by check_conv_desc before any pointer is looked at (int32 indexing) ...
    d = amd._lib.ConvDesc()
    d.N, d.H, d.W, d.Ci, d.Co, d.KH, d.KW, d.stride, d.pad_top, d.pad_left, d.ldx, d.ldy = 2048, 64, 64, 128, 128, 3, 3, 1, 1, 1, 256, 128
    assert 2048 * 64 * 64 * 256 == 1 << 31
    assert lib.vq2_conv_fwd(ctypes.byref(d), 0, None, None, None, None, 0, None, None) == 1
    assert b"exceeds 2^31 elements" in lib.vq2_last_error()
    d.ldx, d.ldy = 128, 256                                    # ... on the output side as well
    assert lib.vq2_conv_dgrad(ctypes.byref(d), 0, None, None, None, 0, None, 0, None, 128, None) == 1
    assert b"exceeds 2^31 elements" in lib.vq2_last_error()
    d.N = 2047                                                 # one image fewer passes check_conv_desc: the next check speaks
    assert lib.vq2_conv_fwd(ctypes.byref(d), 0, None, None, None, None, 0, None, None) == 1
    assert b"null pointer" in lib.vq2_last_error()
    # ... and a conv-transpose to <= 4 channels from 0x7F000000 bytes (its kernel's out-of-range offset) is unsupported:
    # 508 images of 128x128x64 are 0x7F000000 bytes exactly, 507 pass (tests/test_gpu_dispatch.py runs those)
    t = amd._lib.ConvDesc()
    t.N, t.H, t.W, t.Ci, t.Co, t.KH, t.KW, t.stride, t.pad_top, t.pad_left, t.ldx, t.ldy = 508, 128, 128, 64, 4, 4, 4, 2, 1, 1, 64, 4
    t.transposed, t.Cir, t.Cor = 1, 64, 3
    assert 508 * 128 * 128 * 64 * 4 == 0x7F000000
    # (the refusals below come before any launch, but they need non-null, 16-byte aligned pointers: a real host allocation,
    #  so that a regression of a refusal cannot hand a kernel an address nobody owns)
    backing = ctypes.create_string_buffer(4096 + 16)
    dummy = ctypes.c_void_p((ctypes.addressof(backing) + 15) & ~15)
    rc = lib.vq2_conv_fwd(ctypes.byref(t), 0, dummy, dummy, None, None, 0, dummy, None)
    assert rc == 2 and b"limited to tensors below 2130706432 bytes" in lib.vq2_last_error()
    with pytest.raises(RuntimeError, match="split the batch"):
        amd._lib.check(rc, "conv_fwd")
    # the same layer with a residual, ReLU-out or more than 65535 images: its weight panel exists in that kernel's layout only
    t.N = 2
    assert lib.vq2_conv_fwd(ctypes.byref(t), 2, dummy, dummy, None, None, 0, dummy, None) == 2
    assert b"neither a residual nor ReLU-out" in lib.vq2_last_error()
    assert lib.vq2_conv_fwd(ctypes.byref(t), 0, dummy, dummy, None, dummy, 4, dummy, None) == 2
    t.N, t.H, t.W = 65536, 1, 1
    assert lib.vq2_conv_fwd(ctypes.byref(t), 0, dummy, dummy, None, None, 0, dummy, None) == 2
    assert b"65535 images" in lib.vq2_last_error()


def _label_families_in_source():
    """Every kernel label the library can print, tile included, read from csrc/*.hip: the prof_label format strings, and for
    the templated launchers the template arguments in the tile tables (FAST_TILES / GEN_TILES of vq2_conv.hip, the three tables
    of vq2_wino.hip, WGRAD_TILES of vq2_wgrad.hip)."""
    src = {f: open(os.path.join(ROOT, "vq-vae-2-pytorch_amd", "csrc", f)).read()
           for f in os.listdir(os.path.join(ROOT, "vq-vae-2-pytorch_amd", "csrc")) if f.endswith((".hip", ".cpp"))}
    fams = set(m.split("|")[0] for text in src.values() for m in re.findall(r'prof_label\("([^"]+)"', text))
    conv, wino, wgrad = src["vq2_conv.hip"], src["vq2_wino.hip"], src["vq2_wgrad.hip"]
    tiles = {"fast": set(), "gen": set(), "wgrad": set(), "wino": set()}
    for a, b, c, d_, bk in re.findall(r"\bfast_tile<(\d), (\d), (\d), (\d), (\d+)", conv):
        tiles["fast"].add("conv_gemm<%dx%dx%s>" % (int(a) * int(c) * 32, int(b) * int(d_) * 32, bk))
    for a, b, c, d_, bk in re.findall(r"\bgen_tile<(\d), (\d), (\d), (\d), (\d+)", conv):
        tiles["gen"].add("conv_gemm<%dx%dx%s>" % (int(a) * int(c) * 32, int(b) * int(d_) * 32, bk))
    rows = re.findall(r"\bwgrad_tile<(\d), (\d), (\d), (\d)>\(\)", wgrad)
    for a, b, c, d_ in rows:
        tiles["wgrad"].add("wgrad<%dx%d>" % (int(a) * int(c) * 32, int(b) * int(d_) * 32))
    # WGRAD_TILES is the only list: every row once and all of them inside the table, no kernel or launcher instantiated with
    # literal tile arguments anywhere else, no second list of tile dimensions
    table = re.search(r"WGRAD_TILES\[\] = \{(.*?)\n\};", wgrad, re.S).group(1)
    assert len(rows) == len(set(rows)) == len(re.findall(r"\bwgrad_tile<\d", table))
    assert not re.search(r"\b(launch_wgrad|wgrad_kernel|wgrad_fast_kernel)<\d", wgrad)
    assert not re.search(r"\{\d+, \d+\}, \{\d+, \d+\}", wgrad)
    for tpw, nt in re.findall(r"\bwino3_tile<(\d+), (\d), \d+>", wino):
        tiles["wino"].add("conv_wino3<%dx%d,nt%s>" % (64 // int(tpw), 2 * int(tpw), nt))
    for tpw, nt in re.findall(r"\bk4s2_tile<(\d+), (\d), \d+>", wino):
        tiles["wino"].add("conv_wino_k4s2<%dx%d,nt%s>" % (64 // int(tpw), 2 * int(tpw), nt))
    for tpw in re.findall(r"\bsubpixel2_tile<(\d+)>", wino):
        tiles["wino"].add("conv_wino_subpixel<%dx%d>" % (128 // int(tpw), 2 * int(tpw)))
    return fams, tiles


def test_every_kernel_label_in_the_source_has_a_dispatch_case():
    """Census without a GPU: a kernel family or a tile added to csrc/ without a case in tests/test_gpu_dispatch.py fails here.
    (The GPU side of the census asserts that the table really produces EXPECTED_LABELS.)"""
    import test_gpu_dispatch as D
    fams, tiles = _label_families_in_source()
    assert len(tiles["fast"]) == 8 and len(tiles["gen"]) == 5 and len(tiles["wgrad"]) == 6 and len(tiles["wino"]) == 10, tiles
    exp = D.EXPECTED_LABELS
    fam_of = lambda labels: set(l.split("|")[0] for l in labels)
    # every family name (the text before '<' or '|') is covered by the table or is a non-conv family with tests of its own
    covered = set(f.split("<")[0] for f in fam_of(exp["all"] | exp["general"] | D.BIG_LABELS)) | D.OTHER_FAMILIES
    assert set(f.split("<")[0] for f in fams) <= covered, sorted(set(f.split("<")[0] for f in fams) - covered)
    fast = set(l.split("|")[0] for l in exp["all"] if l.startswith("conv_gemm") and not l.endswith("|gen"))
    assert tiles["fast"] == fast, (sorted(tiles["fast"] - fast), sorted(fast - tiles["fast"]))
    gen = set(l.split("|")[0] for l in exp["general"] if l.startswith("conv_gemm"))
    assert tiles["gen"] == gen, (sorted(tiles["gen"] - gen), sorted(gen - tiles["gen"]))
    assert tiles["wino"] == set(l.split("|")[0] for l in exp["all"] if l.startswith("conv_wino"))
    for forms, variant in (("all", "fast"), ("general", "gen")):     # every weight-gradient tile on both kernels
        have = set(l.split("|")[0].replace("sw", "") for l in exp[forms] if l.startswith("wgrad") and l.endswith(variant))
        assert tiles["wgrad"] == have, (forms, sorted(tiles["wgrad"] - have))
    assert {"subpixel_conv|", "conv_k4s2_c4|", "conv1x1_k64|", "convT_small|", "wgrad<128x96>sw|fast", "wgrad<128x32>sw|fast"} <= exp["all"]
    # the literal sets are what the table says, for every value of VQ2_FORMS; every case sits in exactly one place
    for forms, col in (("all", 11), ("direct", 12), ("general", 13)):
        assert set(c[col] for c in D.CASES) == exp[forms], forms
    assert len(set(D.case_id(c) for c in D.CASES)) == len(D.CASES)


def test_dispatch_table_tolerances_bite_on_the_cpu():
    """One small case of every label family of the dispatch table: the comparison with fp64 fails when one product is
    dropped from a plain fp32 computation, and passes without (tests/test_gpu_dispatch.py::_bites; checked for the whole
    table when it was written)."""
    import test_gpu_dispatch as D
    done = set()
    for c in sorted(D.CASES, key=lambda c: c[7] * c[8] * c[9] * c[2] * c[3] * c[4] ** 2):
        fam = c[11].split("|")[0].split("<")[0] + c[0]
        if fam not in done:
            done.add(fam)
            D._bites(c)
    assert len(done) >= 12


def test_geom_dispatch_table_tolerances_bite_on_the_cpu():
    """The same for the table of the same_size form (tests/test_gpu_geom_dispatch.py): the cheapest case of EVERY label
    of EXPECTED_GEOM_LABELS["all"]; and the literal label sets are what the table says, for every value of VQ2_FORMS."""
    import test_gpu_geom_dispatch as G
    for forms, col in (("all", 8), ("direct", 9), ("general", 10)):
        assert set(c[col] for c in G.GEOM_CASES) == G.EXPECTED_GEOM_LABELS[forms], forms
    assert len(set(G.case_id(c) for c in G.GEOM_CASES)) == len(G.GEOM_CASES)
    done = set()
    for c in sorted(G.GEOM_CASES, key=G.cost):
        if c[8] not in done:
            done.add(c[8])
            G._bites(c)
    assert done == G.EXPECTED_GEOM_LABELS["all"]


def test_state_dict_layout_matches_reference(amd):
    m = amd.VQVAE()
    spec = O.state_spec(O.DEFAULT)
    sd = m.state_dict()
    assert list(sd.keys()) == list(spec.keys())
    assert all(tuple(sd[k].shape) == tuple(spec[k]) for k in spec)
    assert m.embed_dim == 128
    live = dict(m.live_named_parameters())
    assert sum(p.numel() for p in live.values()) == 1388867
    assert sum(p.numel() for p in m.parameters()) == 1833092
    m.load_state_dict(O.make_state(O.DEFAULT))      # round-trips a reference-layout checkpoint
    t = amd.VQVAE(channel=32, n_res_block=1, n_res_channel=8, embed_dim=16, n_embed=64)
    assert list(t.state_dict().keys()) == list(O.state_spec(O.TINY).keys())


def test_no_cpu_fallback(amd):
    m = amd.Conv2d(8, 8, 3, padding=1)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(torch.zeros(1, 8, 4, 4))
    with pytest.raises(NotImplementedError):
        amd.ConvTranspose2d(8, 8, 3, stride=1)
    with pytest.raises(ValueError):
        amd.Encoder(3, 32, 1, 8, stride=3)


def test_cycle_scheduler_matches_oracle(amd):
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.Adam([p], lr=3e-4)
    s = amd.CycleScheduler(opt, 3e-4, n_iter=200, momentum=None, warmup_proportion=0.05)
    o = O.CycleSchedule(3e-4, 200, warmup_proportion=0.05)
    for _ in range(450):   # crosses two restarts
        lr, mom = s.step()
        assert mom is None and abs(lr - o.step()) < 1e-15
        assert opt.param_groups[0]["lr"] == lr
    s2 = amd.CycleScheduler(opt, 1e-3, n_iter=10)
    lrs = [s2.step() for _ in range(10)]
    assert abs(lrs[2][0] - 1e-3) < 1e-12 and abs(lrs[2][1] - 0.85) < 1e-12


def test_cycle_scheduler_matches_reference_golden(amd, golden):
    """Trajectories captured from the reference's scheduler.py (oracle/make_golden.py gen_scheduler), for the
    product scheduler AND the oracle's restatement; then an exact resume from state_dict()."""
    from oracle.make_golden_cases import SCHED_CASES
    import numpy as np
    g = golden("scheduler")
    for tag, kw, steps in SCHED_CASES:
        opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
        s = amd.CycleScheduler(opt, **kw)
        lrs, moms = [], []
        for i in range(steps):
            lr, mom = s.step()
            lrs.append(lr)
            moms.append(np.nan if mom is None else mom)
            assert opt.param_groups[0]["lr"] == lr
            assert opt.param_groups[0]["betas"][0] == g[f"{tag}.group_beta1"][i]
        # bit parity: every segment is evaluated with the reference's own expressions (scheduler.py:221-228)
        assert np.array_equal(np.asarray(lrs), g[f"{tag}.lr"]), tag
        assert np.array_equal(np.asarray(moms), g[f"{tag}.momentum"], equal_nan=True), tag
    tag, kw, steps = SCHED_CASES[0]
    o = O.CycleSchedule(kw["lr_max"], kw["n_iter"], warmup_proportion=kw["warmup_proportion"])
    np.testing.assert_allclose([o.step() for _ in range(steps)], g[f"{tag}.lr"], rtol=1e-12, atol=0)
    # resume: 123 steps, save, fresh scheduler, load, continue == uninterrupted
    opt = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=1.0)
    a = amd.CycleScheduler(opt, **kw)
    for _ in range(123):
        a.step()
    b = amd.CycleScheduler(opt, **kw)
    b.load_state_dict(a.state_dict())
    assert np.array_equal(np.asarray([b.step()[0] for _ in range(400)]), g[f"{tag}.lr"][123:523])
    with pytest.raises(ZeroDivisionError):      # the reference divides by an empty warm-up phase on its first step
        amd.CycleScheduler(opt, 1e-3, n_iter=10, warmup_proportion=0.05).step()


def test_code_rows_are_the_reference_pickles(amd, tmp_path):
    """extract_code.py:27-33 / dataset.py:11,36-51: rows are pickle.dumps(CodeRow(top, bottom, filename)) under
    str(index) keys plus a 'length' key.  The expected bytes are built here from the field spec alone."""
    import collections
    import pickle
    import sys
    import types
    import numpy as np
    from vqvae2_amd import codes
    top = np.arange(12, dtype=np.int64).reshape(3, 4)
    bottom = np.arange(48, dtype=np.int64).reshape(6, 8) * 3
    mod = types.ModuleType("dataset")
    mod.CodeRow = collections.namedtuple("CodeRow", ["top", "bottom", "filename"])
    mod.CodeRow.__module__ = "dataset"
    assert "dataset" not in sys.modules
    sys.modules["dataset"] = mod
    try:
        want = pickle.dumps(mod.CodeRow(top=top, bottom=bottom, filename="cls/img_0.png"))
    finally:
        del sys.modules["dataset"]
    got = codes.code_row_bytes(top, bottom, "cls/img_0.png")
    assert got == want and "dataset" not in sys.modules
    path = str(tmp_path / "codes.db")
    with codes.CodeStore(path, "w", backend="sqlite") as st:
        codes.write_code_rows(st, [top, top + 1], [bottom, bottom + 1], ["a/0.png", "a/1.png"], start=0)
        codes.write_code_rows(st, [top + 2], [bottom + 2], ["b/2.png"], start=2)
        st.put(b"length", b"3")
    ds = codes.CodeDataset(path)
    assert len(ds) == 3
    t2, b2, name = ds[2]
    assert name == "b/2.png" and torch.equal(t2, torch.from_numpy(top + 2)) and torch.equal(b2, torch.from_numpy(bottom + 2))
    with codes.CodeStore(path, "r") as st:
        assert st.get(b"1") == codes.code_row_bytes(top + 1, bottom + 1, "a/1.png") and st.get(b"length") == b"3"


def test_code_row_loader_refuses_foreign_globals(amd, tmp_path):
    """A row blob that names anything but dataset.CodeRow / numpy's array rebuild helpers must raise, not run."""
    import pickle
    import numpy as np
    from vqvae2_amd import codes
    marker = tmp_path / "ran"

    class Evil:
        def __reduce__(self):
            return (open, (str(marker), "w"))
    with pytest.raises(pickle.UnpicklingError):
        codes.load_code_row(pickle.dumps(Evil()))
    assert not marker.exists()
    with pytest.raises(pickle.UnpicklingError):      # right container, wrong payload types
        codes.load_code_row(pickle.dumps(("top", "bottom", "name")))
    with pytest.raises(pickle.UnpicklingError):      # object arrays could smuggle arbitrary pickles
        codes.load_code_row(codes.code_row_bytes(np.array([{"a": 1}], dtype=object), np.zeros(2, np.int64), "x"))
    t, b, n = codes.load_code_row(codes.code_row_bytes(np.arange(4), np.arange(6), "k/x.png"))
    assert n == "k/x.png" and t.tolist() == [0, 1, 2, 3] and b.dtype == np.int64


def test_extract_code_preprocessing_uses_torchvision_integer_rules(amd):
    """transforms.Resize(size) truncates the long side (int(size * long / short)) and transforms.CenterCrop(size)
    offsets are int(round((dim - size) / 2.0)) -- hand-computed boxes for odd-sized images (extract_code.py:46-51;
    torchvision itself is not importable here, so these are the formulas' values, not a captured run)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("extract_code_example", os.path.join(ROOT, "examples", "extract_code.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    box = mod.resize_crop_box
    assert box(301, 200, 64) == ((96, 64), (16, 0, 80, 64))           # 64*301/200 = 96.32 -> 96
    assert box(203, 100, 33) == ((66, 33), (16, 0, 49, 33))           # 66.99 truncates to 66 (rounding would say 67)
    assert box(207, 100, 33) == ((68, 33), (18, 0, 51, 33))           # (68-33)/2 = 17.5 -> round -> 18 (floor: 17)
    assert box(100, 206, 33) == ((33, 67), (0, 17, 33, 50))           # 67.98 truncates to 67
    assert box(256, 256, 256) == ((256, 256), (0, 0, 256, 256))


def _check_unsent_slices(trainer_cls):
    import types
    fake = types.SimpleNamespace(arena=types.SimpleNamespace(flat_g=torch.zeros(100)), _sent=[])
    unsent = lambda: trainer_cls._unsent_slices(fake)
    assert unsent() == [(0, 100)]                       # no hook fired: one collective over everything
    fake._sent = [(60, 90)]                             # tail only
    assert unsent() == [(0, 60), (90, 100)]
    fake._sent = [(60, 90), (0, 60)]                    # tail + middle: enc_b's slice is what stays exposed
    assert unsent() == [(90, 100)]
    fake._sent = [(0, 60), (60, 100)]
    assert unsent() == []


def test_unsent_bucket_slices_cover_the_gradient_buffer(amd):
    """Stage1Trainer's fallback after backward: whatever slices the backward hooks did NOT hand to the communicator go
    out then, as maximal contiguous ranges -- never a gap, never a slice twice (no silent un-reduced gradient)."""
    _check_unsent_slices(amd.Stage1Trainer)


def test_stage2_trainer_runs_the_same_unsent_slices(amd):
    """Stage2Trainer reduces the rest of its gradient buffer through the routine pinned above, not a copy of it."""
    _check_unsent_slices(amd.Stage2Trainer)
    assert amd.Stage2Trainer._unsent_slices is amd.Stage1Trainer._unsent_slices


SLOT_SHAPE = (4, 6)
SLOT_KINDS = {"absent": lambda: None, "present": lambda: torch.full(SLOT_SHAPE, 7.0),
              "wrong shape": lambda: torch.full((6, 4), 7.0), "non-contiguous": lambda: torch.full((6, 4), 7.0).t()}


def _slot_case(leaf, grad_set, kind):
    """A CPU tensor in one row of the table: a leaf parameter or the output of an operation on one, with or without .grad,
    `_vq2_grad` attached by hand as ParamArena / planned_weight attach it."""
    p = torch.zeros(SLOT_SHAPE, requires_grad=True)
    if not leaf:
        p = p * 1.0
        if grad_set:
            p.retain_grad()
            p.sum().backward()
    elif grad_set:
        p.grad = torch.ones(SLOT_SHAPE)
    slot = SLOT_KINDS[kind]()
    if slot is not None:
        p._vq2_grad = slot
    assert p.is_leaf == leaf
    if leaf or grad_set:                                # (asking a non-leaf that retains none for .grad warns)
        assert (p.grad is not None) == grad_set
    return p, slot


@pytest.mark.parametrize("kind", list(SLOT_KINDS))
@pytest.mark.parametrize("grad_set", (False, True), ids=("no grad", "grad set"))
@pytest.mark.parametrize("leaf", (True, False), ids=("leaf", "non-leaf"))
def test_gradient_slot_rule_truth_table(amd, leaf, grad_set, kind):
    """ops.slot_of / _grad_slot / landed over (leaf, .grad set, slot): the slot is writable when it is there with the
    parameter's shape and contiguous, and the tensor is no leaf or a leaf without a gradient yet; _grad_slot then hands out
    a NEW tensor on the slot's storage, otherwise a fresh contiguous one; landed() is the pointer comparison of .grad."""
    ops = amd.ops
    p, slot = _slot_case(leaf, grad_set, kind)
    writable = kind == "present" and (not leaf or not grad_set)
    assert (ops.slot_of(p) is slot) if writable else (ops.slot_of(p) is None)
    out = ops._grad_slot(p)
    assert out is not slot and out.shape == p.shape and out.is_contiguous() and out.dtype == p.dtype
    if writable:
        assert out.data_ptr() == slot.data_ptr() and out.untyped_storage().data_ptr() == slot.untyped_storage().data_ptr()
        out.fill_(3.0)
        assert bool((slot == 3.0).all())
    else:
        assert slot is None or out.untyped_storage().data_ptr() != slot.untyped_storage().data_ptr()
        out.fill_(3.0)
        assert slot is None or bool((slot == 7.0).all())
    # landed: whatever .grad holds now is not the slot (a tensor of its own, or nothing)
    if leaf or grad_set:
        assert ops.landed(p) is False
    if leaf and slot is not None:
        p.grad = None
        assert ops.landed(p) is False
        if kind == "present":
            p.grad = slot.view_as(slot)
            assert ops.landed(p) is True
            assert ops.slot_of(p) is None               # ...and a second backward would no longer write there
            p.grad = torch.ones(SLOT_SHAPE)
            assert ops.landed(p) is False


def test_gradient_slot_of_no_parameter(amd):
    assert amd.ops.slot_of(None) is None and amd.ops._grad_slot(None) is None


def test_upload_structs_is_the_arrays_bytes(amd):
    """ops._upload_structs: the device table is the ctypes array byte for byte (here on the CPU)."""
    W = amd._lib.WgradJob
    arr = (W * 2)()
    for i, job in enumerate(arr):
        for j, (name, _) in enumerate(W._fields_):
            if isinstance(getattr(job, name), int):
                setattr(job, name, 1000 * (i + 1) + j)
    raw = bytes(arr)
    assert len(raw) == 2 * ctypes.sizeof(W) and any(raw)
    t = amd.ops._upload_structs(arr, "cpu")
    assert t.dtype == torch.uint8 and t.device.type == "cpu" and t.dim() == 1 and bytes(t.numpy()) == raw
    arr[0].unit_offset = 77                             # a copy, not a window on the ctypes memory
    assert bytes(t.numpy()) == raw


def test_split_checkpoint_recognises_every_accepted_file(amd):
    """What load_state_dict makes of a checkpoint before it touches anything: the model's state_dict without the
    "module." prefix of DDP / DataParallel, and whether optimizer state comes with it."""
    from vqvae2_amd.train import split_checkpoint
    bare = {"conv.weight": torch.ones(2, 2), "conv.bias": torch.zeros(2)}
    prefixed = {"module." + k: v for k, v in bare.items()}
    rest = {"adam_m": torch.zeros(6), "adam_v": torch.zeros(6), "adam_t": 3, "lr": 1e-3, "betas": (0.9, 0.999),
            "scheduler": None}
    for sd, want_full in ((bare, False), (prefixed, False),
                          ({"model": bare, "args": None}, False), ({"model": prefixed, "args": None}, False),
                          (dict(rest, model=bare), True), (dict(rest, model=prefixed), True)):
        model_sd, full = split_checkpoint(sd)
        assert list(model_sd) == list(bare) and full is want_full
        assert all(model_sd[k] is bare[k] for k in bare)


def test_launch_spawns_ranks_and_joins_the_group(amd, tmp_path):
    """distributed.launch (launch.py:22-49) with the gloo backend: two child ranks, environment-first bring-up."""
    out = str(tmp_path / "ranks")
    os.makedirs(out)
    amd.distributed.launch(_launch_probe, 2, 1, 0, "auto", args=(out,), backend="gloo")
    assert sorted(os.listdir(out)) == ["0_of_2_local0", "1_of_2_local1"]


def _launch_probe(out):
    import vqvae2_amd.distributed as d
    x = torch.ones(2) * (d.get_rank() + 1)
    d.all_reduce(x)
    assert float(x[0]) == 3.0
    open(os.path.join(out, f"{d.get_rank()}_of_{d.get_world_size()}_local{d.get_local_rank()}"), "w").close()
    d.synchronize()


def test_distributed_helpers_single_process(amd):
    d = amd.distributed
    assert d.get_world_size() == 1 and d.get_rank() == 0 and d.is_primary()
    x = torch.ones(3)
    assert d.all_reduce(x) is x
    assert d.all_gather({"a": 1}) == [{"a": 1}]
    d.synchronize()
