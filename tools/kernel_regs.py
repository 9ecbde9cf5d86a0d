"""Register / LDS use of the library's kernels, read from the code object embedded in smatrix.so (no GPU needed):
python tools/kernel_regs.py [path/to/smatrix.so] [name filter].  Used to check that a change leaves the instantiations of the
headline path (k_apply_agg<2,1,true,false>, k_apply<0,false>) at their SGPR / VGPR counts -- the residency cliffs of DESIGN.md.
kernel_table(so) gives the same numbers to tests/kernel_budget.py: only the code object's metadata notes are read."""
import os, re, subprocess, sys, tempfile

LIB = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "libsmatrix_amd", "lib", "smatrix.so")
FIELDS = {"sgpr_count": "sgpr", "sgpr_spill_count": "sgpr_spill", "vgpr_count": "vgpr", "vgpr_spill_count": "vgpr_spill",
          "group_segment_fixed_size": "lds", "private_segment_fixed_size": "scratch"}


def strip_args(demangled):
    """'void smx::k_apply<0, false>(smx::Args)' -> 'smx::k_apply<0, false>'; '(anonymous namespace)::k_x(int)' keeps its qualifier:
    the cut is at the parenthesis that matches the LAST one, not at the first"""
    s = demangled.strip()
    if s.endswith(")"):
        depth = 0
        for i in range(len(s) - 1, -1, -1):
            depth += (s[i] == ")") - (s[i] == "(")
            if depth == 0:
                s = s[:i]
                break
    return s[5:] if s.startswith("void ") else s


def code_object(so_path):
    d = open(so_path, "rb").read()
    i = 0
    while True:
        i = d.find(b"\x7fELF", i)
        if i < 0: raise RuntimeError("no gfx code object found in %s" % so_path)
        if int.from_bytes(d[i + 18:i + 20], "little") == 224: break      # EM_AMDGPU
        i += 4
    shoff = int.from_bytes(d[i + 40:i + 48], "little"); size = shoff + int.from_bytes(d[i + 58:i + 60], "little") * int.from_bytes(d[i + 60:i + 62], "little")
    return d[i:i + size]


def kernel_table(so_path=LIB):
    """{demangled kernel name without its argument list, never cut: {sgpr, sgpr_spill, vgpr, vgpr_spill, lds, scratch}}, in the
    code object's order; one llvm-readelf and one c++filt process"""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code_object(so_path)); f.flush()
        notes = subprocess.run(["/opt/rocm/lib/llvm/bin/llvm-readelf", "--notes", f.name], capture_output=True, text=True, check=True).stdout
    cur = {}
    rows = []
    for line in notes.splitlines():
        m = re.match(r"\s+\.(name|%s):\s+(\S+)" % "|".join(FIELDS), line)
        if not m: continue
        if m.group(1) in cur: rows.append(cur); cur = {}
        cur[m.group(1)] = m.group(2)
    if cur: rows.append(cur)
    for r in rows:
        if len(r) != len(FIELDS) + 1: raise RuntimeError("incomplete kernel metadata: %r" % r)
    demangled = subprocess.run(["c++filt"], input="".join(r["name"] + "\n" for r in rows), capture_output=True, text=True, check=True).stdout.splitlines()
    if len(demangled) != len(rows): raise RuntimeError("c++filt answered %d lines for %d names" % (len(demangled), len(rows)))
    table, mangled = {}, {}
    for r, d in zip(rows, demangled):
        name = strip_args(d)
        if name in table: raise RuntimeError("%s and %s both demangle to %s" % (mangled[name], r["name"], name))
        mangled[name] = r["name"]
        table[name] = {short: int(r[key]) for key, short in FIELDS.items()}
    return table


if __name__ == "__main__":
    table = kernel_table(sys.argv[1] if len(sys.argv) > 1 else LIB)
    flt = sys.argv[2] if len(sys.argv) > 2 else ""
    width = max([48] + [len(n) for n in table if flt in n])
    for name, r in table.items():
        if flt in name:
            print("%-*s sgpr %3s (spilled %2s)  vgpr %3s (spilled %s)  lds %s  scratch %s" % (width, name, r["sgpr"], r["sgpr_spill"], r["vgpr"], r["vgpr_spill"], r["lds"], r["scratch"]))
