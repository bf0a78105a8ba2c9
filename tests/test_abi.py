"""libbfhip.so loads and exports exactly the ABI of include/bfhip.h (CPU only;
no compute calls need a GPU here)."""
import ctypes
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bfhip.h")


def declared_functions():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(bf_[a-z_0-9]+)\s*\(", src)))


def test_header_functions_listed_in_binding(pkg):
    assert set(declared_functions()) == set(pkg._lib.SIGNATURES), \
        "include/bfhip.h and _lib.SIGNATURES disagree"


def header_arity():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(bf_[a-z_0-9]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


RUBY_DRIVERS = os.path.join(ROOT, "redis-bloomfilter_amd", "ruby", "lib", "bloomfilter_driver")


def test_ruby_ffi_binding_matches_header():
    """redis-bloomfilter_amd/ruby/.../hip*.rb attach only declared functions, with the right arity
    (Ruby is not installed here, so this static check stands in for running it)."""
    rb = open(os.path.join(RUBY_DRIVERS, "hip.rb")).read()
    lua_rb = open(os.path.join(RUBY_DRIVERS, "hip_lua.rb")).read()
    arity = header_arity()
    attached = re.findall(r"attach_function :(bf_\w+),\s*(%i\[[^\]]*\]|\[[^\]]*\])", rb + lua_rb)
    assert len(attached) >= 24
    for name, args in attached:
        assert name in arity, name
        if args.startswith("%i["):
            n = len(args[3:-1].split())
        else:
            inner = args[1:-1].strip()
            n = 0 if not inner else inner.count(",") + 1
        assert n == arity[name], (name, n, arity[name])
    # the FFI struct layout lists bf_config's fields in order
    cfg = re.search(r"typedef struct bf_config \{(.*?)\} bf_config;", open(HEADER).read(), re.S).group(1)
    cfg = re.sub(r"/\*.*?\*/", "", cfg, flags=re.S)
    fields = re.findall(r"\b(?:uint32_t|int32_t|uint64_t)\s+(\w+)(?:\[\w+\])?;", cfg)
    layout = re.findall(r":(\w+), (?::u?int\d+|\[:u?int\d+, \w+\])", re.search(r"layout (.*?)\n\s*end", rb, re.S).group(1))
    assert layout == fields
    assert "devices" in fields


def _ruby_methods(src):
    """(name, params, body lines with their line numbers) of every `def` in a Ruby file,
    a method ending at the first `end` indented like its `def`."""
    lines = src.splitlines()
    out = []
    i = 0
    while i < len(lines):
        m = re.match(r"^(\s*)def (?:self\.)?(\w+[?!=]?)\s*(?:\((.*)\))?\s*$", lines[i])
        if not m:
            i += 1
            continue
        indent, name, params = m.group(1), m.group(2), m.group(3) or ""
        j = i + 1
        while j < len(lines) and not re.match(r"^%send\b" % re.escape(indent), lines[j]):
            j += 1
        out.append((name, params, [(n + 1, lines[n]) for n in range(i + 1, j)]))
        i = j + 1
    return out


def _split_args(s):
    """Top-level comma split of an argument list."""
    depth, cur, args = 0, "", []
    for ch in s:
        if ch in "([{":
            depth += 1
        elif ch in ")]}":
            depth -= 1
        if ch == "," and depth == 0:
            args.append(cur.strip())
            cur = ""
        else:
            cur += ch
    if cur.strip():
        args.append(cur.strip())
    return args


def _ffi_calls(line):
    """(function, [args]) of every HipFFI / HipLuaFFI call on a line (balanced parentheses)."""
    for m in re.finditer(r"\bHip(?:Lua)?FFI\.(bf_\w+)\(", line):
        depth, k = 1, m.end()
        while k < len(line) and depth:
            depth += {"(": 1, ")": -1}.get(line[k], 0)
            k += 1
        yield m.group(1), _split_args(line[m.end():k - 1])


def test_ruby_ffi_calls_are_well_formed():
    """Every FFI call in the Ruby drivers passes as many arguments as the C prototype takes, and
    every local it names is bound before the call in the same method (a parameter, an earlier
    assignment or block parameter) or is a method of the drivers — Ruby is absent here, so this
    static check stands in for running them (it catches e.g. an unbound `len`, a NameError)."""
    arity = header_arity()
    srcs = {fn: open(os.path.join(RUBY_DRIVERS, fn)).read() for fn in ("hip.rb", "hip_lua.rb", "hip_test.rb")}
    methods = {name for src in srcs.values() for name, _, _ in _ruby_methods(src)}
    literals = {"nil", "true", "false", "self"}
    ncalls = 0
    for fn, src in srcs.items():
        for name, params, body in _ruby_methods(src):
            bound = {p.strip().lstrip("*&").split("=")[0].split(":")[0].strip() for p in params.split(",") if p.strip()}
            for lineno, line in body:
                code = line.split(" #")[0]
                for fname, args in _ffi_calls(code):
                    ncalls += 1
                    where = "%s:%d %s" % (fn, lineno, fname)
                    assert fname in arity, where
                    assert len(args) == arity[fname], (where, args)
                    for a in args:
                        root = re.match(r"^[a-z_]\w*", a)
                        if not root or root.group(0) in literals:
                            continue   # literal, constant, @ivar or expression on one of them
                        assert root.group(0) in bound or root.group(0) in methods, \
                            "%s: '%s' is not bound in %s" % (where, root.group(0), name)
                # assignments (incl. `a, b = ...`) and block parameters bind for later lines
                lhs = re.match(r"^\s*([a-z_][\w\s,]*?)\s*(?:\|\|)?=(?!=|~)", code)
                if lhs:
                    bound |= {v.strip() for v in lhs.group(1).split(",")}
                for blk in re.findall(r"\|([^|]+)\|", code):
                    bound |= {v.strip() for v in blk.split(",")}
    assert ncalls >= 25


def test_library_exports_every_symbol(pkg):
    lib = pkg._lib.load()
    for name in declared_functions():
        assert hasattr(lib, name), name
    out = subprocess.run(["nm", "-D", "--defined-only", pkg._lib.lib_path()], capture_output=True, text=True)
    exported = set(re.findall(r"\bT (bf_\w+)", out.stdout))
    assert set(declared_functions()) <= exported


def test_library_is_gfx950_only(pkg):
    blob = open(pkg._lib.lib_path(), "rb").read()
    targets = set(re.findall(rb"amdgcn-amd-amdhsa--(gfx[0-9a-z]+)", blob))
    assert targets == {b"gfx950"}


# The only environment knobs the shipped library reads: path choices the GPU tests force (every
# one gives identical results) and the host staging thread count.  An experiment's A/B knob
# (BF_AB_GETENV / ab_u32) exists only in -DBFHIP_AB_KNOBS builds (tools/build_ab_libs.sh) and
# leaves the tree once DESIGN §6f records its verdict — VERDICT r04 item 2.
PRODUCT_KNOBS = {"BFHIP_INSERT_BINNED", "BFHIP_INCLUDE_BINNED", "BFHIP_BIN_REGION_LOG2",
                 "BFHIP_SHARD_TEST_BINNED", "BFHIP_CHUNK_TEST_L2", "BFHIP_ROUTE_AGG", "BFHIP_HOST_THREADS"}


def test_library_reads_only_path_knobs(pkg):
    blob = open(pkg._lib.lib_path(), "rb").read()
    knobs = {m.decode() for m in re.findall(rb"BFHIP_[A-Z0-9_]+", blob)}
    assert knobs == PRODUCT_KNOBS, sorted(knobs ^ PRODUCT_KNOBS)


def test_version(pkg):
    assert pkg.version().startswith("bfhip ")


def test_sizing_helpers_match_facade(pkg, oracle):
    for n, p in [(1000, 0.01), (100, 0.02), (10**9, 0.01), (2 * 10**11, 1e-4), (3, 0.9)]:
        m = pkg._lib.optimal_m(n, p)
        assert m == oracle.optimal_m(n, p) == pkg.Bloomfilter.optimal_m(n, p)
        assert pkg._lib.optimal_k(n, m) == oracle.optimal_k(n, m) == pkg.Bloomfilter.optimal_k(n, m)


def test_optimal_m_non_finite_is_an_error(pkg):
    """error_rate 0 -> Infinity: the reference raises FloatDomainError (Float#round); the ABI
    returns BF_OPTIMAL_M_INVALID instead of casting Infinity to int64."""
    assert pkg._lib.load().bf_optimal_m(100.0, 0.0) == pkg._lib.BF_OPTIMAL_M_INVALID
    assert pkg._lib.load().bf_optimal_m(float("nan"), 0.01) == pkg._lib.BF_OPTIMAL_M_INVALID
    with pytest.raises(FloatingPointError):
        pkg._lib.optimal_m(100, 0.0)


def test_invalid_arguments_without_gpu(pkg):
    """Argument checks run before any device call (and map to ArgumentError)."""
    with pytest.raises(pkg.ArgumentError, match="m_bits == 0"):
        pkg.Filter(0, 6)
    with pytest.raises(pkg.ArgumentError, match="k must be"):
        pkg.Filter(100, 0)
    with pytest.raises(pkg.ArgumentError, match="k must be"):
        pkg.Filter(100, 65)
    # bf_indexes (one key, no filter): m = 0 is the reference's ZeroDivisionError (ruby.rb:51)
    with pytest.raises(pkg.ArgumentError, match="m and k must be positive"):
        pkg._lib.indexes(b"asdlol", 0, 6)
    with pytest.raises(pkg.ArgumentError, match="m and k must be positive"):
        pkg._lib.indexes(b"asdlol", 9585, 0)
    with pytest.raises(pkg.ArgumentError, match="k must be in"):
        pkg._lib.indexes(b"asdlol", 9585, 65)


def test_null_handle_is_einval(pkg):
    lib = pkg._lib.load()
    assert lib.bf_clear(None) == pkg._lib.BF_EINVAL
    assert lib.bf_destroy(None) == 0
    assert lib.bf_insert_many(None, None, None, 0, None, None) == pkg._lib.BF_EINVAL


def test_no_device_is_reported_loudly(pkg):
    """On a machine without a GPU the engine refuses to run (no CPU fallback)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(pkg.BfHipError, match="BF_EDEVICE"):
        pkg.Filter(9585, 6)


def test_product_does_not_import_oracle():
    """The product package never imports, links or execs oracle/."""
    pkg_dir = os.path.join(ROOT, "redis-bloomfilter_amd")
    for dirpath, _, files in os.walk(pkg_dir):
        for fn in files:
            if fn.endswith((".py", ".cpp", ".hip", ".h", ".rb", "Makefile")):
                text = open(os.path.join(dirpath, fn), errors="replace").read()
                assert "bf_oracle" not in text and "import oracle" not in text and "libbforacle" not in text, fn
    lib = os.path.join(pkg_dir, "lib", "libbfhip.so")
    out = subprocess.run(["readelf", "-d", lib], capture_output=True, text=True)
    assert "bforacle" not in out.stdout


def test_bfbench_binary_is_built_and_reports_its_version():
    """The C++ bench binary links libbfhip.so; --version needs no GPU."""
    import subprocess
    exe = os.path.join(ROOT, "redis-bloomfilter_amd", "lib", "bfbench")
    out = subprocess.run([exe, "--version"], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and out.stdout.startswith("bfhip ")


def test_check_offsets_is_the_kernels_rule(pkg):
    """bf_check_offsets applies bfdev::key_ok, the rule every hashing kernel checks per key
    before it hashes: non-decreasing offsets, every key below 2 GiB.
    A wrapped length (round 5's hang: a key end read back as 0) is refused, not looped over."""
    import numpy as np
    pkg._lib.check_offsets(np.array([0, 3, 3, 10, 4096], np.uint64))
    pkg._lib.check_offsets(np.array([7], np.uint64))                     # n = 0
    with pytest.raises(pkg.ArgumentError, match="key 1:"):
        pkg._lib.check_offsets(np.array([0, 5, 2, 9], np.uint64))       # 5 -> 2 runs backwards
    with pytest.raises(pkg.ArgumentError, match="key 0:"):
        pkg._lib.check_offsets(np.array([0, 5, 9, 0], np.uint64))       # the r05 wrap: the end read as 0
        #                                                                 (every key then passes the last offset)
    with pytest.raises(pkg.ArgumentError, match="key 0:"):
        pkg._lib.check_offsets(np.array([0, 1 << 31], np.uint64))       # a 2 GiB key
    pkg._lib.check_offsets(np.array([0, (1 << 31) - 1], np.uint64))
    # the kernels carry the same guard and report through the handle's key-status word
    blob = open(pkg._lib.lib_path(), "rb").read()
    assert b"key offsets were inconsistent" in blob
