"""Per-kernel register / scratch / spill table from hipcc -Rpass-analysis=kernel-resource-usage
(compile-time check, no GPU).  python tools/regs.py [filter] [file.hip ...]  (default conv.hip; each file is
built device-only with build.py's flags for it)"""
import importlib.util, os, re, subprocess, sys, tempfile
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(HERE, "inference-time-scaling-for-diffusion-models-beyond-scaling-denoising-steps_amd")
spec = importlib.util.spec_from_file_location("itsd_build", os.path.join(PKG, "build.py"))
build = importlib.util.module_from_spec(spec)
spec.loader.exec_module(build)
flt = sys.argv[1] if len(sys.argv) > 1 else ""
srcs = [a for a in sys.argv[2:]] or ["conv.hip"]
for s in srcs:
    src = os.path.join(build.CSRC, s)
    with tempfile.TemporaryDirectory() as tmp:
        cmd = [build.HIPCC] + build.flags_for(src) + ["--cuda-device-only", "-c", src, "-o", os.path.join(tmp, "regs.o"),
                                                       "-Rpass-analysis=kernel-resource-usage"]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.exit(r.stderr)
    cur = None
    rows = {}
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
            rows[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?):\s+(\d+)", line)
        if m and cur:
            rows[cur][m.group(1).strip()] = int(m.group(2))
    for k, v in rows.items():
        if flt in k:
            print(f"{k[:70]:70s} vgpr {v.get('VGPRs',0):3d} agpr {v.get('AGPRs',0):3d} scratch {v.get('ScratchSize [bytes/lane]',0):4d} "
                  f"vspill {v.get('VGPRs Spill',0):3d} sspill {v.get('SGPRs Spill',0):3d} sgpr {v.get('TotalSGPRs',0):3d} "
                  f"lds {v.get('LDS Size [bytes/block]',0):6d} occ {v.get('Occupancy [waves/SIMD]',0)}")
