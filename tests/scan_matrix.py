"""Every instantiation of the scan kernels (kmp_scan_stream.hip, kmp_scan_general.hip, kmp_scan_multi.hip) and the call that launches it.
Plain Python: no GPU, no torch, nothing of the package.

A row is keyed by the kernel's demangled name without `void`, `(anonymous namespace)::` and the parameter list, as `normalise`
writes it: "kmp_scan_flat_kernel<6, false, false>".  tests/test_scan_matrix_host.py holds ROWS and UNREACHABLE to the symbols the
compiler emits (both directions), tests/test_gpu_scan_matrix.py runs every row against the CPU oracle and the host model, and
its trace test shows that the kernel a row names is the kernel that ran.  A new instantiation in a launcher therefore fails the host
test until it has a row here, and the row fails the trace test until its options really reach the kernel.

The three files hold 118 instantiations: 26 streaming + 36 general + 56 fused.  98 have a row; the launchers cannot pick the other 20.

The dispatch, quoted from the launch code (c = the context, s = the pattern set of the pass, a = kmp_scan_args):

  kmpgpu.hip
    use_flat(c):    c->uniform && c->mode == 0 && (c->kernel_sel == 3 || (c->kernel_sel == 0 && (c->uni_len >= 512u || !c->packed || !c->bitmap_live)))
    use_fused(c,s): c->packed && c->bitmap_live && c->mode == 0 && c->kernel_sel != 1 && !s.fused_groups.empty() && c->fused != 0 && s.n_multi_unique >= 2
    use_packed(c):  c->packed && c->bitmap_live && c->mode == 0 && (c->kernel_sel == 2 || ((c->kernel_sel == 0 || c->kernel_sel == 3) && !use_flat(c)))
    pad_clean:      prepare_packed: own || dirty == 0 -- an arena of the library's own (kmpgpu_load_arena) has its padding cleared, a
                    borrowed one (kmpgpu_attach_arena) is clean only when kmp_check_padding_kernel finds every padding byte 0x00
    enqueue_set:    the fused groups of the set first (kmp_launch_scan_multi, one launch per group), then what keeps a pass of its own in
                    two groups, {>= 4 bytes: a.masked = false} and {< 4 bytes: a.masked = true}:
                    flat ? kmp_launch_scan_flat : packed ? kmp_launch_scan_packed : kmp_launch_scan
                    a.depth = c->depth, a.mode = c->mode, a.nontemporal = c->nontemporal != 0, a.whole = c->whole_payload != 0;
                    a pass that emits (kmpgpu_scan_offsets, kmpgpu_scan_packets) refuses the general kernel
  kmp_scan_stream.hip
    kmp_launch_scan_flat:   switch (a.depth) { case 2, 3, 5, 6, 8: launch_flat_t<that>; default: launch_flat_t<4> }
    launch_flat_t<DEPTH>:   a.whole ? (kmp_emits(a) ? flat_whole<4, true, true> : a.nontemporal ? flat_whole<4, true> : flat_whole<4, false>)
                            : kmp_emits(a) ? flat<4, true, true> : a.nontemporal ? flat<DEPTH, true> : flat<DEPTH, false>
    kmp_launch_scan_packed: switch (a.depth) { case 2: case 3: launch_packed_t<3>; case 6: case 8: launch_packed_t<6>; default: launch_packed_t<4> }
    launch_packed_t<DEPTH>: as launch_flat_t
  kmp_scan_general.hip
    kmp_launch_scan:        a.mode == 1 ? launch_scan_d<true, 1> : a.masked ? launch_scan_d<true, 0> : launch_scan_d<false, 0>
    launch_scan_d:          switch (a.depth) { case 2, 3, 5, 6: launch_scan_t<that>; default: launch_scan_t<4> }
    launch_scan_t<DEPTH>:   a.whole ? kmp_scan_kernel<4, MASKED, MODE, a.nontemporal, true> : kmp_scan_kernel<DEPTH, MASKED, MODE, a.nontemporal>
  kmp_scan_multi.hip (K = kmp_scan_multi_kernel, KW = .._wide_kernel, KE = .._emit_kernel, or their _whole twins under a.whole; all <3, NT, CLEAN, ONES, CLASSED>)
    kmp_multi_kind(emit, pad_clean, n_ones): emit ? 2 : (n_ones != 0u || !pad_clean) ? 1 : 0        (0 = K, 1 = KW, 2 = KE)
    kmp_launch_scan_multi:  if (kmp_emits(a)) KMP_MULTI_LAUNCH(true, true, a.pad_clean)              -- an emitting pass is always NT = true
                            else KMP_MULTI_LAUNCH(false, a.nontemporal, a.pad_clean)
    KMP_MULTI_LAUNCH_K:     classed ? (EMIT ? KE<NT, CLEAN, false, true> : !CLEAN ? KW<NT, CLEAN, false, true> : K<NT, true, false, true>)
                            : EMIT ? (n_ones ? KE<NT, CLEAN, true, false> : KE<NT, CLEAN, false, false>)
                            : n_ones ? KW<NT, CLEAN, true, false> : !CLEAN ? KW<NT, CLEAN, false, false> : K<NT, true, false, false>
    (kmp_tables.cpp: up to 256 distinct patterns of 2..99 bytes are one plain group; more: the 2-byte ones -- or, with 1-byte
    patterns riding along, the first 256 -- fill plain groups and the rest classed groups; up to four 1-byte patterns ride with the first group)
"""
import re

# KMPGPU_OPT_* by name, and what kmpgpu_set_option accepts for each (kmpgpu.hip; the host test looks for these refusals' messages there)
OPTIONS = {"MODE": 1, "BLOCKS_PER_CU": 2, "DEPTH": 3, "FUSED": 4, "KERNEL": 5, "NONTEMPORAL": 100, "WHOLE_PAYLOAD": 9}
ACCEPTED = {"MODE": {0, 1}, "BLOCKS_PER_CU": set(range(0, 257)), "DEPTH": {0, 2, 3, 4, 5, 6, 8}, "FUSED": {0, 1, 2}, "KERNEL": {0, 1, 2, 3},
            "NONTEMPORAL": {0, 1}, "WHOLE_PAYLOAD": {0, 1}}
REFUSALS = ("mode must be 0 or 1", "blocks per CU must be 0 (auto) or 1..256", "depth must be 0 (auto), 2..6 or 8", "fused must be 0, 1 or 2",
            "kernel selection must be 0, 1, 2 or 3", "whole payload must be 0")
KERNEL_AUTO, KERNEL_GENERAL, KERNEL_PACKED, KERNEL_FLAT = 0, 1, 2, 3

ARENAS = ("uniform", "mixed", "borrowed_dirty", "uniform_dirty")
PATTERNS = ("long", "short", "riders", "classed")
CALLS = ("scan", "scan_packets", "scan_offsets")
SOURCES = ("kmp_scan_stream.hip", "kmp_scan_general.hip", "kmp_scan_multi.hip")


def normalise(name):
    """a demangled kernel name (c++filt, or the Kernel_Name column of a kernel trace) as the table writes it"""
    name = name.strip().strip('"')
    name = re.sub(r"^void\s+", "", name).replace("(anonymous namespace)::", "")
    name = re.sub(r"\(.*$", "", name)                                   # the parameter list (and " [clone .kd]")
    name = re.sub(r"\s*\[clone.*$|\.kd$", "", name)
    name = re.sub(r"\s*,\s*", ", ", name)
    return name.strip()


def is_scan_kernel(name):
    """an instantiation of the three files' scan kernels (kmp_scan_local_kernel and kmp_scan_totals_kernel of kmp_prep.hip are prefix sums)"""
    return re.match(r"kmp_scan_(kernel|(flat|packed)(_whole)?_kernel|multi(_whole)?(_wide|_emit)?_kernel)<", name) is not None


def _b(x):
    return "true" if x else "false"


def _row(name, family, options, arena, patterns, call, also=(), nocase=False):
    return {"name": name, "family": family, "options": dict(options), "arena": arena, "patterns": patterns, "call": call, "also": tuple(also),
            "nocase": nocase}


def _streaming():
    """flat: a uniform arena under KERNEL_FLAT; packed: any packed arena under KERNEL_PACKED; FUSED = 0 keeps multi-pattern sets here.
    The `short` set has 1-, 2- and 3-byte patterns beside long ones: both launch groups (`a.masked` is unused by these kernels)."""
    rows = []
    for fam, sel, depths, arenas in (("flat", KERNEL_FLAT, (2, 3, 4, 5, 6, 8), ("uniform", "uniform_dirty")),
                                     ("packed", KERNEL_PACKED, (3, 4, 6), ("mixed", "borrowed_dirty"))):
        base = {"KERNEL": sel, "FUSED": 0}
        for d in depths:
            for nt in (1, 0):
                # the arena kind alternates, so that either kind meets both cache policies and, over the depths, every ring
                rows.append(_row(f"kmp_scan_{fam}_kernel<{d}, {_b(nt)}, false>", fam, {**base, "DEPTH": d, "NONTEMPORAL": nt},
                                 arenas[(d + nt) % 2], "short", "scan", nocase=(d == 4 and not nt)))
        rows.append(_row(f"kmp_scan_{fam}_kernel<4, true, true>", fam, base, arenas[1], "short", "scan_packets"))
        for nt in (1, 0):                                               # (DEPTH is set and must be ignored: whole payloads run four chunks deep)
            rows.append(_row(f"kmp_scan_{fam}_whole_kernel<4, {_b(nt)}, false>", fam, {**base, "WHOLE_PAYLOAD": 1, "NONTEMPORAL": nt, "DEPTH": 6},
                             arenas[nt], "short", "scan", nocase=bool(nt)))
        rows.append(_row(f"kmp_scan_{fam}_whole_kernel<4, true, true>", fam, {**base, "WHOLE_PAYLOAD": 1}, arenas[1], "short", "scan_offsets"))
    return rows


def _general():
    """KERNEL_GENERAL; MODE = 1 is the automaton (launch_scan_d<true, 1> whatever the patterns' lengths).  A `short` set under MODE = 0
    launches MASKED = false for its long patterns and MASKED = true for its short ones; a `long` set MASKED = false alone."""
    rows = []
    for d in (2, 3, 4, 5, 6):
        for nt in (1, 0):
            o = {"KERNEL": KERNEL_GENERAL, "DEPTH": d, "NONTEMPORAL": nt}
            arena = ("mixed", "borrowed_dirty")[(d + nt) % 2]
            other = ("mixed", "borrowed_dirty")[(d + nt + 1) % 2]
            plain = f"kmp_scan_kernel<{d}, false, 0, {_b(nt)}, false>"
            rows.append(_row(plain, "general", o, arena, "long", "scan"))
            rows.append(_row(f"kmp_scan_kernel<{d}, true, 0, {_b(nt)}, false>", "general", o, other, "short", "scan", also=(plain,), nocase=(d == 3)))
            rows.append(_row(f"kmp_scan_kernel<{d}, true, 1, {_b(nt)}, false>", "general", {**o, "MODE": 1}, arena, "short", "scan"))
    for nt in (1, 0):
        o = {"KERNEL": KERNEL_GENERAL, "WHOLE_PAYLOAD": 1, "NONTEMPORAL": nt, "DEPTH": 5}            # (DEPTH as for the streaming twins)
        arena = ("mixed", "borrowed_dirty")[nt]
        plain = f"kmp_scan_kernel<4, false, 0, {_b(nt)}, true>"
        rows.append(_row(plain, "general", o, arena, "long", "scan"))
        rows.append(_row(f"kmp_scan_kernel<4, true, 0, {_b(nt)}, true>", "general", o, arena, "short", "scan", also=(plain,)))
        rows.append(_row(f"kmp_scan_kernel<4, true, 1, {_b(nt)}, true>", "general", {**o, "MODE": 1}, arena, "short", "scan", nocase=bool(nt)))
    return rows


def _fused():
    """FUSED = 1 on a packed arena.  CLEAN follows the arena (mixed: the library's own copy; borrowed_dirty: attached, padding kept), ONES the
    1-byte riders, CLASSED the group.  A classed set runs its plain first group (the 2-byte patterns) before the classed ones: `also`."""
    rows = []
    for whole in (0, 1):
        w = "_whole" if whole else ""
        for nt in (1, 0):
            o = {"KERNEL": KERNEL_AUTO, "FUSED": 1, "NONTEMPORAL": nt, "WHOLE_PAYLOAD": whole}

            def k(kind, clean, ones, classed):
                return f"kmp_scan_multi{w}{kind}_kernel<3, {_b(nt)}, {_b(clean)}, {_b(ones)}, {_b(classed)}>"
            rows.append(_row(k("", 1, 0, 0), "fused", o, "mixed", "long", "scan", nocase=bool(whole and nt)))
            rows.append(_row(k("", 1, 0, 1), "fused", o, "mixed", "classed", "scan", also=(k("", 1, 0, 0),)))
            rows.append(_row(k("_wide", 1, 1, 0), "fused", o, "mixed", "riders", "scan"))
            rows.append(_row(k("_wide", 0, 1, 0), "fused", o, "borrowed_dirty", "riders", "scan", nocase=not (whole or nt)))
            rows.append(_row(k("_wide", 0, 0, 0), "fused", o, "borrowed_dirty", "long", "scan"))
            rows.append(_row(k("_wide", 0, 0, 1), "fused", o, "borrowed_dirty", "classed", "scan", also=(k("_wide", 0, 0, 0),)))
        # the emitting passes: NT = true whatever KMPGPU_OPT_NONTEMPORAL says -- half of the rows say 0
        for clean, arena in ((1, "mixed"), (0, "borrowed_dirty")):
            def e(ones, classed):
                return f"kmp_scan_multi{w}_emit_kernel<3, true, {_b(clean)}, {_b(ones)}, {_b(classed)}>"
            o = {"KERNEL": KERNEL_AUTO, "FUSED": 1, "WHOLE_PAYLOAD": whole, "NONTEMPORAL": clean}
            rows.append(_row(e(0, 0), "fused", o, arena, "long", "scan_packets" if clean else "scan_offsets", nocase=bool(clean and not whole)))
            rows.append(_row(e(1, 0), "fused", o, arena, "riders", "scan_offsets" if clean else "scan_packets"))
            rows.append(_row(e(0, 1), "fused", o, arena, "classed", "scan_packets" if clean != whole else "scan_offsets", also=(e(0, 0),)))
    return rows


ROWS = _streaming() + _general() + _fused()
BY_NAME = {r["name"]: r for r in ROWS}


def _unreachable():
    """name -> the launcher line (kmp_scan_multi.hip, kmp_launch_scan_multi) that keeps it from being picked.  KMP_MULTI_LAUNCH_K expands
    every branch at each of its six call sites, the ones whose condition is a constant false there included."""
    out = {}
    for w in ("", "_whole"):
        for clean in (1, 0):
            for ones, classed in ((0, 0), (1, 0), (0, 1)):
                out[f"kmp_scan_multi{w}_emit_kernel<3, false, {_b(clean)}, {_b(ones)}, {_b(classed)}>"] = \
                    "`if (EMIT_K_)` inside KMP_MULTI_LAUNCH(false, false, CLEAN_): EMIT_K_ is false wherever NT_ is -- " \
                    "`if (kmp_emits(a)) { ... KMP_MULTI_LAUNCH(true, true, ...) }` is the only emitting call site"
        for nt in (1, 0):
            for classed in (0, 1):
                out[f"kmp_scan_multi{w}_wide_kernel<3, {_b(nt)}, true, false, {_b(classed)}>"] = \
                    ("`else if (!(CLEAN_)) KMP_MULTI_LAUNCH0(KW_, NT_, CLEAN_, false, true)`" if classed else
                     "`else if (!(CLEAN_)) KMP_MULTI_LAUNCH1(KW_, NT_, CLEAN_, false)`") + " inside KMP_MULTI_LAUNCH(.., .., true): !(CLEAN_) is false there"
    return out


UNREACHABLE = _unreachable()
