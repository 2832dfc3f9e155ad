"""In-tree build of libvorbispizza_synth.so (hipcc, gfx950 only).

The built library lives in vorbispizza_amd/lib/ (git-ignored, but shipped to the GPU box by
gpurun).  No JIT cache, no torch extension machinery: plain `hipcc -shared -fPIC`.
"""
import os
import subprocess
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_DIR = os.path.join(_HERE, "lib")
LIB_PATH = os.path.join(LIB_DIR, "libvorbispizza_synth.so")
OBJ_DIR = os.path.join(LIB_DIR, "obj")

# translation unit -> extra flags.  imdct_exact.hip and the host-side table / state-machine code
# must round every f32 multiply/add separately, like the reference's JIT output.
SOURCES = {
    "imdct_fast.hip": [],
    "imdct_exact.hip": ["-ffp-contract=off"],
    "synth_kernels.hip": [],
    "synth_dual.hip": [],
    "synth_pairs.hip": [],   # synth_dual.hip once more, for channel pairs of streams with 4, 6, 8, ... channels
    "steady_stereo.hip": [],  # the stereo fast path's second kernel: batches of steady long frames, overlap-added in the lanes
    "synth_big.hip": [],
    "floor0.hip": ["-ffp-contract=off"],
    "vpz_context.hip": ["-ffp-contract=off"],
    "vpz_decoder.hip": ["-ffp-contract=off"],
    "synth_plan.hip": ["-ffp-contract=off"],   # the host plan of a synth call: pass 1 and the run cutting, integers only
    "entropy.hip": ["-ffp-contract=off"],  # the residue sums: plain adds in the CPU front end's order
    "pcm_pack.hip": [],  # vpz_pcm_pack: windows of a device PCM array as a padded batch (a copy: no arithmetic)
    "pcm_resample.hip": [],  # vpz_pcm_resample: the same delivery at one sample rate (float32 multiply-adds, fused: the tolerance covers them)
    "pcm_logmel.hip": [],  # vpz_pcm_logmel: windows of a mono device array as (log-)mel frames (the DFT on the exact float32 MFMA)
    "pcm_melspec.hip": ["-ffp-contract=off"],  # vpz_pcm_melspec: the same frames with transforms of 2048, 4096 and 8192: a real FFT in LDS, one transform per frame (every fused step is written as one)
    "pcm_stft.hip": ["-ffp-contract=off"],  # vpz_pcm_stft: the spectrum itself -- complex, magnitude or power -- of rows of a float32 array, transforms of 512 to 8192: the same real FFT, two or four frames side by side at the small sizes
    "pcm_cqt.hip": ["-ffp-contract=off"],  # vpz_pcm_cqt: rows of a float32 array as constant-Q spectrograms: one kernel per bin, a framed matrix product on the exact float32 MFMA whose dead k-ranges are skipped per block of 32 bins
    "pcm_fbank.hip": [],  # vpz_pcm_fbank: the same windows as Kaldi filterbank frames (per-frame mean, the folded operator on the same MFMA); vpz_pcm_mfcc: the same tile core with the cepstral stage
    "pcm_loudness.hip": [],  # vpz_pcm_loudness: windows of an interleaved device array as K-weighted step sums and a peak (float64; the recurrence cut into steps, carried exactly)
    "pcm_truepeak.hip": [],  # vpz_pcm_true_peak: the same windows' true peak (a 4x / 2x polyphase interpolator in float32, fused, one order) and sample peak; range and maxima of step sums, host only
    "pcm_featpost.hip": ["-ffp-contract=off"],  # vpz_feat_post: deltas and mean / variance normalisation of a padded batch of feature frames (every fused step is written as one)
    "pcm_normalize.hip": ["-ffp-contract=off"],  # vpz_pcm_normalize: windows of a planar float32 array delivered normalised -- unit variance, peak, RMS or a gain --: ordered float64 chunk sums, then the values as two float32 operations, never fused
}
COMMON = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-function",
          "-Wno-constant-logical-operand", "-fno-strict-aliasing"]


def _hipcc():
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return "hipcc"


def _deps(src):
    deps = [src]
    if os.path.basename(src) == "synth_pairs.hip":
        deps.append(os.path.join(CSRC, "synth_dual.hip"))
    for name in os.listdir(CSRC):
        if name.endswith(".hpp"):
            deps.append(os.path.join(CSRC, name))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_synth.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_entropy.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_entropy_group.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_pcm.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_pcm_pack.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_pcm_resample.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_pcm_logmel.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_pcm_melspec.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_pcm_stft.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_pcm_cqt.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_pcm_fbank.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_pcm_mfcc.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_pcm_loudness.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_pcm_r128.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_pcm_featpost.h"))
    deps.append(os.path.join(_HERE, "..", "include", "vorbispizza_pcm_normalize.h"))
    return deps


HOST_DIR = os.path.join(_HERE, "host")
HOST_LIB_PATH = os.path.join(LIB_DIR, "libvorbispizza_host.so")


def build_host(force=False, verbose=False):
    """Compile the C++ host side with g++: the CPU front end (Ogg + Vorbis setup + entropy decode) and
    the VorbisReader / StreamDecoder.Read mirror, which calls the C ABI of libvorbispizza_synth.so."""
    os.makedirs(LIB_DIR, exist_ok=True)
    srcs = [os.path.join(HOST_DIR, "vorbis_front.cpp"), os.path.join(HOST_DIR, "vorbis_reader.cpp"),
            os.path.join(HOST_DIR, "vorbis_multi.cpp")]
    inc = os.path.join(_HERE, "..", "include")
    deps = srcs + [os.path.join(inc, "vorbispizza_front.h"), os.path.join(inc, "vorbispizza_reader.h"),
                   os.path.join(inc, "vorbispizza_multi.h"), os.path.join(inc, "vorbispizza_synth.h"),
                   os.path.join(inc, "vorbispizza_entropy.h"), os.path.join(inc, "vorbispizza_entropy_group.h"),
                   os.path.join(inc, "vorbispizza_multi_mixed.h"), os.path.join(inc, "vorbispizza_multi_ranges.h"),
                   os.path.join(inc, "vorbispizza_pcm.h"), os.path.join(inc, "vorbispizza_pcm_pack.h"),
                   os.path.join(inc, "vorbispizza_multi_batch.h"), os.path.join(inc, "vorbispizza_pcm_resample.h"),
                   os.path.join(inc, "vorbispizza_multi_resample.h"), os.path.join(inc, "vorbispizza_pcm_logmel.h"),
                   os.path.join(inc, "vorbispizza_multi_logmel.h"), os.path.join(inc, "vorbispizza_pcm_fbank.h"),
                   os.path.join(inc, "vorbispizza_multi_fbank.h"), os.path.join(inc, "vorbispizza_pcm_loudness.h"),
                   os.path.join(inc, "vorbispizza_multi_loudness.h"), os.path.join(inc, "vorbispizza_pcm_r128.h"),
                   os.path.join(inc, "vorbispizza_multi_r128.h"), os.path.join(inc, "vorbispizza_pcm_mfcc.h"),
                   os.path.join(inc, "vorbispizza_multi_mfcc.h"), os.path.join(inc, "vorbispizza_pcm_featpost.h"),
                   os.path.join(inc, "vorbispizza_multi_featpost.h"), os.path.join(inc, "vorbispizza_pcm_melspec.h"),
                   os.path.join(inc, "vorbispizza_multi_melspec.h"), os.path.join(inc, "vorbispizza_pcm_stft.h"),
                   os.path.join(inc, "vorbispizza_multi_stft.h"), os.path.join(inc, "vorbispizza_pcm_cqt.h"),
                   os.path.join(inc, "vorbispizza_multi_cqt.h"), os.path.join(inc, "vorbispizza_pcm_normalize.h"),
                   os.path.join(inc, "vorbispizza_multi_normalize.h"), LIB_PATH]
    stale = force or not os.path.exists(HOST_LIB_PATH) or any(
        os.path.exists(d) and os.path.getmtime(d) > os.path.getmtime(HOST_LIB_PATH) for d in deps)
    if stale:
        cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall", "-pthread",
               "-o", HOST_LIB_PATH] + srcs + ["-L" + LIB_DIR, "-lvorbispizza_synth", "-Wl,-rpath,$ORIGIN"]
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    return HOST_LIB_PATH


def build(force=False, verbose=False):
    """Compile every HIP translation unit for gfx950 and link the C-ABI shared library, then the
    C++ host library that sits above it."""
    os.makedirs(OBJ_DIR, exist_ok=True)
    hipcc = _hipcc()
    # (diagnostic builds: VPZ_EXTRA_HIPCC_FLAGS=-DVPZ_STAMPS; a change of flags rebuilds everything)
    extra_env = os.environ.get("VPZ_EXTRA_HIPCC_FLAGS", "")
    flags_file = os.path.join(OBJ_DIR, "flags.txt")
    if (open(flags_file).read() if os.path.exists(flags_file) else "") != extra_env:
        force = True
        with open(flags_file, "w") as f:
            f.write(extra_env)
    objs, relink, jobs = [], force or not os.path.exists(LIB_PATH), []
    for name, extra in SOURCES.items():
        src = os.path.join(CSRC, name)
        if not os.path.exists(src):
            raise RuntimeError("missing source " + src)
        obj = os.path.join(OBJ_DIR, name.replace(".hip", ".o"))
        stale = force or not os.path.exists(obj) or any(
            os.path.getmtime(d) > os.path.getmtime(obj) for d in _deps(src))
        if stale:
            jobs.append([hipcc] + COMMON + extra + extra_env.split() + ["-c", src, "-o", obj])
            relink = True
        objs.append(obj)
    if jobs:  # the translation units are independent: compile them side by side (a handful of hipcc processes)
        from concurrent.futures import ThreadPoolExecutor

        def compile_one(cmd):
            if verbose:
                print(" ".join(cmd), flush=True)
            subprocess.run(cmd, check=True)

        with ThreadPoolExecutor(max_workers=min(len(jobs), max(1, (os.cpu_count() or 2) // 2))) as pool:
            list(pool.map(compile_one, jobs))
    if relink:
        cmd = [hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB_PATH] + objs
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True)
    build_host(force, verbose)
    return LIB_PATH


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
