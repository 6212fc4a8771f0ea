"""Per-kernel register / scratch / occupancy summary of libsparc_amp's HIP
source (hipcc -Rpass-analysis=kernel-resource-usage), with each kernel's
kernel-argument segment size and kernarg preload length (the dwords of leading
plain parameters that arrive in SGPRs with the wave) read back from the code
object, filtered by a regex on the demangled name:
  python scripts/kres.py 'k_secb<float, 8, 4' [source.hip [hipcc args ...]]
The unit that csrc/Makefile builds with the preload flag (sa_row2.hip) gets it
here too.

  python scripts/kres.py --lib [libsparc_amp.so [regex]]
reads a built library instead (no compile): kernarg size and preload length of
every kernel in it (library_kernels, which tests/test_kernarg_head_host.py
imports)."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/llvm/bin"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=16"]
PRELOAD_UNITS = ("sa_row2.hip",)
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def demangle(names):
    names = list(names)
    if not names:
        return {}
    dem = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
    return dict(zip(names, dem))


def library_kernels(lib):
    """{mangled kernel name: (kernarg size in bytes, preload length in dwords)}
    of every gfx950 kernel in a built library, from its kernel descriptors."""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        fat = os.path.join(tmp, "fat.bin")
        subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(tmp, "copy.so")],
                       check=True)
        blob = open(fat, "rb").read()
        starts = [m.start() for m in re.finditer(re.escape(MAGIC), blob)]
        for i, s in enumerate(starts):  # one bundle per translation unit
            part, co = os.path.join(tmp, f"b{i}.bin"), os.path.join(tmp, f"b{i}.elf")
            open(part, "wb").write(blob[s:starts[i + 1] if i + 1 < len(starts) else len(blob)])
            subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o",
                            "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--input={part}", f"--output={co}"], check=True)
            dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "-j", ".rodata", co], capture_output=True, text=True,
                                 check=True).stdout
            cur = None
            for line in dis.splitlines():
                t = line.split()
                if len(t) == 2 and t[0] == ".amdhsa_kernel":
                    cur = t[1]
                    out[cur] = [0, 0]
                elif cur and len(t) == 2 and t[0] == ".amdhsa_kernarg_size":
                    out[cur][0] = int(t[1])
                elif cur and len(t) == 2 and t[0] == ".amdhsa_user_sgpr_kernarg_preload_length":
                    out[cur][1] = int(t[1])
    return {k: tuple(v) for k, v in out.items()}


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--lib":
        lib = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "sparc_ldpc_amd", "libsparc_amp.so")
        pat = re.compile(sys.argv[3] if len(sys.argv) > 3 else ".")
        ks = library_kernels(lib)
        names = demangle(ks)
        for k, (size, pre) in sorted(ks.items(), key=lambda kv: names.get(kv[0], kv[0])):
            if pat.search(names.get(k, k)):
                print(f"{names.get(k, k)[:110]:110s} kernarg {size:4d} B preload {pre:2d}")
        return
    pat = re.compile(sys.argv[1] if len(sys.argv) > 1 else ".")
    src = sys.argv[2] if len(sys.argv) > 2 else "sparc_ldpc_amd/csrc/sparc_amp.hip"
    extra = sys.argv[3:]
    if os.path.basename(src) in PRELOAD_UNITS:
        extra = PRELOAD + extra
    cache = "/tmp/kres_remarks.txt"
    if os.environ.get("KRES_CACHED") and os.path.exists(cache):
        err = open(cache).read()
    else:
        err = subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared",
                              "-Iinclude", "-fno-slp-vectorize", "-Rpass-analysis=kernel-resource-usage", "-o",
                              "/tmp/kres.so", src] + extra, capture_output=True, text=True).stderr
        open(cache, "w").write(err)
    cur, rows = None, {}
    for line in err.splitlines():
        m = re.search(r"remark:\s+(.*?)\s+\[-Rpass", line)
        if not m:
            continue
        txt = m.group(1)
        if txt.startswith("Function Name:"):
            cur = txt.split(":", 1)[1].strip()
            rows[cur] = {}
        elif cur and ":" in txt:
            k, v = txt.split(":", 1)
            rows[cur][k.strip()] = v.strip()
    names = demangle(rows)
    args = library_kernels("/tmp/kres.so") if os.path.exists("/tmp/kres.so") else {}
    for k, d in rows.items():
        nm = names.get(k, k)
        if pat.search(nm):
            size, pre = args.get(k, ("?", "?"))
            print(f"{nm[:90]:90s} VGPR {d.get('VGPRs', '?'):>4s} AGPR {d.get('AGPRs', '?'):>3s} "
                  f"SGPR {d.get('TotalSGPRs', '?'):>4s} scratch {d.get('ScratchSize [bytes/lane]', '?'):>4s} "
                  f"occ {d.get('Occupancy [waves/SIMD]', '?')} kernarg {size:>4} B preload {pre:>2}")


if __name__ == "__main__":
    main()
