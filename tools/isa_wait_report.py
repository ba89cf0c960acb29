"""Static picture of how a kernel's MFMAs sit behind its LDS reads (host only: hipcc cross-compiles, nothing runs on a GPU).

    python tools/isa_wait_report.py [--filter REGEX] [--list] coskad_amd/csrc/fused_bwd.hip [more .hip files]

Each file is compiled to gfx950 assembly with the CXXFLAGS of coskad_amd/csrc/Makefile (+ --cuda-device-only -S).  Per kernel:
registers, scratch, occupancy (the compiler's own footer), the number of MFMAs and of LDS waits, and the histogram of MFMAs issued
between consecutive LDS waits.  An LDS wait is an `s_waitcnt` with an lgkmcnt field; `zero` / `one` are the waits with no / exactly
one MFMA before the next wait, `7+` those with seven or more.  `exposed` counts the MFMAs that stand behind a wait for an LDS read
issued after the previous MFMA: a full LDS round trip in front of that MFMA, in an in-order wave.  (A counted lgkmcnt(N) leaves the
N youngest reads in flight; they are not held against the MFMA.)  --list prints the assembly line of every exposed MFMA.
Only v_mfma*, ds_read* and s_waitcnt are looked at; the counts are static, so a rolled loop counts once."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "coskad_amd", "csrc")


def makefile_flags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    var = dict(re.findall(r"^(\w+)\s*\??=\s*(.*)$", text, re.M))
    flags = re.sub(r"\$\((\w+)\)", lambda m: var.get(m.group(1), ""), var["CXXFLAGS"])
    return os.environ.get("HIPCC", var.get("HIPCC", "hipcc")), flags.split()


def compile_asm(path, extra, keep):
    hipcc, flags = makefile_flags()
    if keep:
        os.makedirs(keep, exist_ok=True)
        out = os.path.join(os.path.abspath(keep), os.path.splitext(os.path.basename(path))[0] + ".s")
    else:
        out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    subprocess.run([hipcc] + flags + extra + ["--cuda-device-only", "-S", os.path.abspath(path), "-o", out], check=True, cwd=CSRC)
    text = open(out).read()
    if not keep:
        os.unlink(out)
    return text


def demangle(names):
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            res = subprocess.run([tool] + names, capture_output=True, text=True, check=True).stdout.split("\n")
            return {n: re.sub(r"^void |\(.*$", "", d).replace("coskad::", "").replace(" ", "") for n, d in zip(names, res)}
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def scan(text):
    """-> {mangled name: record}"""
    kernels, cur = {}, None
    for n, line in enumerate(text.split("\n"), 1):
        t = line.strip()
        m = re.match(r"^(_Z\w+):", t)
        if m and cur is None:
            cur = dict(mfma=0, gaps=[], since=None, reads=[], retired=False, exposed=[], foot={})
            kernels[m.group(1)] = cur
            continue
        if cur is None:
            continue
        op = t.split()[0] if t else ""
        if op.startswith("v_mfma"):
            cur["mfma"] += 1
            if cur["since"] is not None:
                cur["since"] += 1
            if cur["retired"]:
                cur["exposed"].append(n)
            cur["retired"] = False
            cur["reads"] = [False] * len(cur["reads"])       # reads still in flight were issued before this MFMA
        elif op.startswith("ds_read"):
            cur["reads"].append(True)                        # True: issued after the previous MFMA
        elif op == "s_waitcnt":
            m = re.search(r"lgkmcnt\((\d+)\)", t)
            if m:
                if cur["since"] is not None:
                    cur["gaps"].append(cur["since"])
                cur["since"] = 0
                keep = int(m.group(1))
                done = cur["reads"][:len(cur["reads"]) - keep] if keep < len(cur["reads"]) else []
                if any(done):
                    cur["retired"] = True
                cur["reads"] = cur["reads"][len(done):]
        elif t.startswith("; ") and ":" in t:
            k, _, v = t[2:].partition(":")
            if k in ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize"):
                cur["foot"][k] = v.split()[0]
                if k == "Occupancy":                         # the last footer line of interest: the kernel is complete
                    cur = None
    return kernels


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("files", nargs="+")
    ap.add_argument("--filter", default=None, help="only kernels whose demangled name matches this regular expression")
    ap.add_argument("--list", action="store_true", help="print the assembly line numbers of the exposed MFMAs")
    ap.add_argument("--keep", default=None, metavar="DIR", help="keep the assembly files there (the lines --list names)")
    ap.add_argument("-D", action="append", default=[], help="extra -D definitions for the compile")
    a = ap.parse_args()
    print(f"{'kernel':44s} {'vgpr':>4s} {'agpr':>4s} {'scratch':>7s} {'occ':>3s} {'mfma':>5s} {'waits':>5s} {'zero':>5s} {'one':>5s} "
          f"{'2-6':>5s} {'7+':>5s} {'exposed':>7s}")
    for path in a.files:
        kernels = scan(compile_asm(path, ["-D" + d for d in a.D], a.keep))
        names = demangle(list(kernels))
        print(f"# {os.path.relpath(os.path.abspath(path), ROOT)}")
        for k, r in sorted(kernels.items(), key=lambda kv: names[kv[0]]):
            if r["mfma"] == 0 or (a.filter and not re.search(a.filter, names[k])):
                continue
            g, f = r["gaps"], r["foot"]
            print(f"{names[k][:44]:44s} {f.get('NumVgprs', '?'):>4s} {f.get('NumAgprs', '?'):>4s} {f.get('ScratchSize', '?'):>7s} "
                  f"{f.get('Occupancy', '?'):>3s} {r['mfma']:5d} {len(g):5d} {sum(x == 0 for x in g):5d} {sum(x == 1 for x in g):5d} "
                  f"{sum(2 <= x <= 6 for x in g):5d} {sum(x >= 7 for x in g):5d} {len(r['exposed']):7d}")
            if a.list and r["exposed"]:
                print("    exposed MFMAs at lines " + " ".join(map(str, r["exposed"])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
