"""Compare the gfx950 kernels of two builds of libnerf_hip.so (CPU only).

    python tools/kernel_diff.py OLD.so NEW.so [--md profiles/NAME.md] [--relaid PATTERN ...]

For every kernel: the bytes of its function symbol, its 64-byte kernel descriptor and
its metadata record (VGPR, AGPR, SGPR, scratch, spills, static LDS), old against new.
Kernels are matched by demangled name; the chunk-major fp32 kernels, whose template
lists lost their constant parameters (mlp_fwd_kernel<PREC, XB, DB, TRAIN, TPW, G, NT> ->
<XB, DB, TRAIN>, mlp_bwd_kernel<PREC, XB, DB, TPW, G, NT, WX> -> <XB, DB, WX>), are
matched by the parameters they kept.  Exit status 1 if a matched kernel differs or a
kernel is missing on either side, other than those given with --gone PATTERN.  A kernel
given with --relaid PATTERN (its argument struct was laid out anew, so its kernarg offsets
and code bytes move) passes when its VGPR, AGPR, scratch, spill and static-LDS figures
match; its SGPR count and code size are reported."""

from __future__ import annotations

import argparse
import hashlib
import re
import subprocess
import sys
import tempfile
from pathlib import Path

LLVM = Path("/opt/rocm/lib/llvm/bin")
# what a kernel whose arguments were laid out anew must keep (--relaid)
KEPT = ("vgpr_count", "agpr_count", "private_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
        "group_segment_fixed_size")
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count",
          "sgpr_spill_count", "group_segment_fixed_size")


def run(*cmd, cwd=None) -> str:
    return subprocess.run([str(c) for c in cmd], check=True, capture_output=True, text=True, cwd=cwd).stdout


def role(demangled: str) -> str:
    """Name a kernel by what it computes, whichever template list it was built with."""
    name = demangled.split("(")[0]
    m = re.fullmatch(r"void nr::mlp_fwd_kernel<(\d+), (\d+), (\d+), (\w+), 1, 8, 256>", name)
    if m and m.group(1) == "0":
        return f"void nr::mlp_fwd_kernel<{m.group(2)}, {m.group(3)}, {m.group(4)}>"
    m = re.fullmatch(r"void nr::mlp_bwd_kernel<(\d+), (\d+), (\d+), 1, 10, 256, (\w+)>", name)
    if m and m.group(1) == "0":
        return f"void nr::mlp_bwd_kernel<{m.group(2)}, {m.group(3)}, {m.group(4)}>"
    return name


def kernels(lib: Path) -> dict:
    """{role: {"code": sha1, "bytes": n, "kd": sha1, <FIELDS>...}} over every code object of lib."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        (Path(tmp) / "k.so").write_bytes(lib.read_bytes())
        run(LLVM / "llvm-objdump", "--offloading", "k.so", cwd=tmp)
        for co in sorted(Path(tmp).glob("k.so.*gfx950*")):
            blob = co.read_bytes()
            secs = {}
            for ln in run(LLVM / "llvm-readelf", "-SW", co).splitlines():
                m = re.match(r"\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", ln)
                if m:
                    secs[int(m.group(1))] = (int(m.group(3), 16), int(m.group(4), 16))  # address, file offset
            syms = {}
            for ln in run(LLVM / "llvm-readelf", "-sW", co).splitlines():
                f = ln.split()
                if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
                    addr, off = secs[int(f[6])]
                    start = int(f[1], 16) - addr + off
                    syms[f[7]] = blob[start:start + int(f[2])]
            # the metadata note: one "  - .key: value" / "    .key: value" record per kernel
            # (its arguments' records are indented deeper)
            meta, cur = {}, {}
            for ln in run(LLVM / "llvm-readelf", "--notes", co).splitlines() + ["  - .end: 0"]:
                m = re.match(r"  (- |  )\.(\w+):\s+(\S+)", ln)
                if not m:
                    continue
                if m.group(1) == "- ":
                    if "name" in cur:
                        meta[cur["name"]] = {f: int(cur[f]) for f in FIELDS if f in cur}
                    cur = {}
                cur[m.group(2)] = m.group(3)
            for sym, code in syms.items():
                if sym + ".kd" not in syms:
                    continue
                # the descriptor without kernel_code_entry_byte_offset (bytes 16..23: where the
                # code sits relative to the descriptor, a property of the object's layout)
                kd = syms[sym + ".kd"]
                rec = {"code": hashlib.sha1(code).hexdigest(), "bytes": len(code),
                       "kd": hashlib.sha1(kd[:16] + kd[24:]).hexdigest(), **meta.get(sym, {})}
                out[role(run("c++filt", sym).strip())] = rec
    return out


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--md", help="write the table as markdown")
    ap.add_argument("--gone", action="append", default=[], help="regex of kernels expected only in OLD")
    ap.add_argument("--relaid", action="append", default=[],
                    help="regex of kernels whose code may differ while their register, scratch and LDS figures match")
    args = ap.parse_args()
    old, new = kernels(Path(args.old)), kernels(Path(args.new))
    rows, bad = [], 0
    for k in sorted(set(old) | set(new)):
        o, n = old.get(k), new.get(k)
        if o and n:
            same = all(o.get(f) == n.get(f) for f in ("code", "kd", *FIELDS))
            what = ", ".join([f"bytes {o['bytes']} -> {n['bytes']}"] +
                             [f"{f} {o.get(f)} -> {n.get(f)}" for f in FIELDS if o.get(f) != n.get(f)])
            kept = any(re.search(p, k) for p in args.relaid) and all(o.get(f) == n.get(f) for f in KEPT)
            verdict = "identical" if same else ("resources match: " if kept else "DIFFERS: ") + what
            bad += not (same or kept)
        elif o:
            expected = any(re.search(p, k) for p in args.gone)
            verdict = "removed" if expected else "MISSING in new"
            bad += not expected
        else:
            verdict = "ONLY in new"
            bad += 1
        r = n or o
        rows.append((k.replace("void nr::", ""), r["bytes"], r.get("vgpr_count"), r.get("agpr_count"),
                     r.get("sgpr_count"), r.get("private_segment_fixed_size"),
                     (r.get("vgpr_spill_count") or 0) + (r.get("sgpr_spill_count") or 0),
                     r.get("group_segment_fixed_size"), verdict))
    both = [r for r in rows if r[-1] == "identical" or r[-1].startswith(("DIFFERS", "resources match"))]
    gone = [r for r in rows if r[-1] == "removed"]
    lines = ["| kernel | bytes | VGPR | AGPR | SGPR | scratch | spills | static LDS | old vs new |",
             "|---|---|---|---|---|---|---|---|---|"]
    lines += ["| `" + r[0] + "` | " + " | ".join(str(x) for x in r[1:]) + " |" for r in rows]
    total = (f"{len(both)} kernels in both builds, {sum(r[-1] == 'identical' for r in both)} byte-identical "
             f"(code, kernel descriptor, metadata), "
             f"{sum(r[-1].startswith('resources match') for r in both)} with matching resources and new code, "
             f"{sum(r[1] for r in both)} bytes of machine code; "
             f"{len(gone)} removed ({sum(r[1] for r in gone)} bytes); "
             f"{sum(r[-1] in ('ONLY in new', 'MISSING in new') for r in rows)} unmatched.")
    text = "\n".join(lines) + "\n\n" + total + "\n"
    if args.md:
        Path(args.md).write_text(text)
    print(text)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
