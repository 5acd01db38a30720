"""Did a re-filing of code change the device code?  python tools/kernel_diff.py OLD.so NEW.so [--show NAME]

Extracts the gfx950 code objects of two builds of the library (on copies: llvm-objdump --offloading writes beside its input) and compares,
for every kernel present in both, (1) the resource notes (VGPR, SGPR, AGPR, scratch, LDS, kernarg size, spills) and (2) the disassembled
instruction stream with what depends on where the kernel was linked taken out: addresses, encodings, symbol offsets, and the literal of
the pc-relative address pairs (s_getpc_b64 + s_add_u32 / s_addc_u32).  Prints the kernels that differ, those only in one library, and
exits 1 if any kernel differs.  --show NAME prints a unified diff of the normalised streams of the kernels whose name contains NAME."""
import difflib, glob, os, re, shutil, subprocess, sys, tempfile

LLVM = os.environ.get("SRW_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
CXXFILT = shutil.which("llvm-cxxfilt", path=LLVM) or shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or sys.exit("needs llvm-cxxfilt or c++filt")
NOTE_KEYS = ("vgpr_count", "sgpr_count", "agpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "kernarg_segment_size",
             "vgpr_spill_count", "sgpr_spill_count", "max_flat_workgroup_size", "uses_dynamic_stack")


def run(*cmd):
    return subprocess.run(cmd, capture_output=True, text=True, check=True).stdout


def normalise(lines):
    out, pcrel = [], 0
    for ln in lines:
        ln = ln.split("//")[0].rstrip()                      # address and encoding
        ln = re.sub(r"\s*<[^>]*>\s*$", "", ln)               # symbol + offset of a branch target
        if not ln.strip() or ln.strip() == "...":            # (...: the zero padding behind a kernel)
            continue
        ins = ln.split()
        if ins[0] == "s_getpc_b64":
            pcrel = 4                                        # the add / addc pair follows within a few instructions
        elif pcrel and ins[0] in ("s_add_u32", "s_addc_u32", "s_add_i32", "s_sub_u32", "s_subb_u32") and re.match(r"^(0x[0-9a-f]+|-?\d+)$", ins[-1]):
            ln = " ".join(ins[:-1] + ["<pcrel>"])
        pcrel = max(0, pcrel - 1)
        out.append(" ".join(ln.split()))
    return out


def kernels_of(lib):
    """name -> list of (notes, normalised instruction stream), one per code object that holds a kernel of that name"""
    tmp = tempfile.mkdtemp()
    try:
        dst = os.path.join(tmp, os.path.basename(lib))
        shutil.copy(lib, dst)
        subprocess.run([LLVM + "/llvm-objdump", "--offloading", dst], capture_output=True, check=True)
        found = {}
        for co in sorted(glob.glob(dst + ".*gfx950*")):
            notes = {}
            for blk in run(LLVM + "/llvm-readelf", "--notes", co).split("- .agpr_count")[1:]:
                blk = ".agpr_count" + blk
                get = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "-"])[1]
                notes[get("name")] = tuple((k, get(k)) for k in NOTE_KEYS)
            cur, body = None, {}
            for ln in run(LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", co).splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:$", ln)
                if m:
                    cur = m.group(1)
                    body[cur] = []
                elif cur is not None:
                    body[cur].append(ln)
            # keyed by the demangled name without "(anonymous namespace)::": a record type that moved into a header renames every
            # kernel that takes it, and is no change of code
            names = list(notes)
            plain = subprocess.run([CXXFILT], input="\n".join(names) + "\n", capture_output=True, text=True, check=True).stdout.splitlines()
            for name, key in zip(names, plain):
                found.setdefault(key.replace("(anonymous namespace)::", ""), []).append((notes[name], normalise(body.get(name, []))))
        for v in found.values():
            v.sort()
        return found
    finally:
        shutil.rmtree(tmp)


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    show = sys.argv[sys.argv.index("--show") + 1] if "--show" in sys.argv else None
    if show is not None:
        args.remove(show)
    if len(args) != 2:
        sys.exit(__doc__)
    old, new = kernels_of(os.path.abspath(args[0])), kernels_of(os.path.abspath(args[1]))
    both = sorted(set(old) & set(new))
    differ = []
    for name in both:
        if old[name] == new[name]:
            continue
        what = []
        if [o[0] for o in old[name]] != [n[0] for n in new[name]]:
            what.append("resources " + ", ".join("%s %s -> %s" % (k, a, b) for (k, a), (_, b) in zip(old[name][0][0], new[name][0][0]) if a != b))
        if [o[1] for o in old[name]] != [n[1] for n in new[name]]:
            what.append("instructions (%d -> %d)" % (sum(len(o[1]) for o in old[name]), sum(len(n[1]) for n in new[name])))
        differ.append(name)
        print("DIFFERS  %s: %s" % (name, "; ".join(what)))
        if show is not None and show in name:
            sys.stdout.writelines(l + "\n" for l in difflib.unified_diff(old[name][0][1], new[name][0][1], "old", "new", lineterm="", n=2))
    for name in sorted(set(old) - set(new)):
        print("ONLY OLD %s" % name)
    for name in sorted(set(new) - set(old)):
        print("ONLY NEW %s" % name)
    empty = [n for n in both if not all(o[1] for o in old[n]) or not all(x[1] for x in new[n])]
    if empty:
        sys.exit("no instructions found for: %s" % ", ".join(empty))
    print("%d kernels in both, %d differ; %d only in the old library, %d only in the new" %
          (len(both), len(differ), len(set(old) - set(new)), len(set(new) - set(old))))
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
