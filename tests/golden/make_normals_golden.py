"""Writes tests/golden/normals.npz: inputs and outputs of the reference's own normal-map kernels
(lib/normals/compute_normals.cu:30-101, computeVmapKernel + computeNmapKernel), the pin of tests/normals_ref.py and of
the device-side normal map.

    POSECNN_REFERENCE=<root of the PoseCNN reference tree> python tests/golden/make_normals_golden.py

The two kernel bodies are cut out of the reference file when this runs (nothing of them is kept here), written into a
temporary directory next to a small driver, compiled by g++ against the stand-ins of oracle/ref_shim/
(eigen_sophus_on_cpu.h: the thread indices and Eigen's 3-vector with its published evaluation order; read only) and run
with the thread indices swept serially, one "thread" per pixel, the vertex map first and the normal map after it, as
compute_normals() launches them (1.f / fx and 1.f / fy formed there). No FMA contraction (-ffp-contract=off): the
canonical arithmetic of this repository. Arrays only; two frames, 12 x 20 and 19 x 37."""
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
FIRST, LAST = 30, 101   # the lines of the two __global__ functions

DRIVER = r"""
#include "eigen_sophus_on_cpu.h"
static inline float __int_as_float(int i) { float f; std::memcpy(&f, &i, 4); return f; }
static inline bool isnan(float x) { return x != x; }
#include "kernels.inc"
int main(int argc, char** argv)
{
  FILE* in = std::fopen(argv[1], "rb");
  int hw[2];
  float k[5];
  if (!in || std::fread(hw, 4, 2, in) != 2 || std::fread(k, 4, 5, in) != 5) return 1;
  const int H = hw[0], W = hw[1];
  std::vector<float> depth((size_t)H * W), vmap((size_t)H * W * 3), nmap((size_t)H * W * 3);
  if (std::fread(depth.data(), 4, depth.size(), in) != depth.size()) return 1;
  std::fclose(in);
  const float fx_inv = 1.f / k[0], fy_inv = 1.f / k[1];
  for (int u = 0; u < H; u++)
    for (int v = 0; v < W; v++) {
      blockIdx.x = v; blockIdx.y = u;
      computeVmapKernel(depth.data(), vmap.data(), fx_inv, fy_inv, k[2], k[3], k[4], H, W);
    }
  for (int u = 0; u < H; u++)
    for (int v = 0; v < W; v++) {
      blockIdx.x = v; blockIdx.y = u;
      computeNmapKernel(vmap.data(), nmap.data(), H, W);
    }
  FILE* out = std::fopen(argv[2], "wb");
  if (!out || std::fwrite(nmap.data(), 4, nmap.size(), out) != nmap.size()) return 1;
  std::fclose(out);
  return 0;
}
"""


def build(reference_root, tmp):
    path = os.path.join(reference_root, "lib", "normals", "compute_normals.cu")
    lines = open(path).read().split("\n")[FIRST - 1:LAST]
    assert lines[0].startswith("__global__ void computeVmapKernel") and lines[-1] == "}", "the reference file is not the one expected"
    assert sum(l.startswith("__global__") for l in lines) == 2
    with open(os.path.join(tmp, "kernels.inc"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    with open(os.path.join(tmp, "driver.cpp"), "w") as fh:
        fh.write(DRIVER)
    exe = os.path.join(tmp, "driver")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + tmp,
                           os.path.join(tmp, "driver.cpp"), "-o", exe])
    return exe


def run(exe, tmp, depth, intrinsics, cutoff):
    H, W = depth.shape
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(fin, "wb") as fh:
        fh.write(np.array([H, W], np.int32).tobytes())
        fh.write(np.concatenate([intrinsics, [cutoff]]).astype(np.float32).tobytes())
        fh.write(np.ascontiguousarray(depth, np.float32).tobytes())
    subprocess.check_call([exe, fin, fout])
    return np.fromfile(fout, np.float32).reshape(H, W, 3)


def frame(rng, H, W, cutoff):
    """A tilted, rippled surface with a constant-depth plane, zero holes, values at and above the cutoff, and a NaN."""
    yy, xx = np.mgrid[0:H, 0:W]
    d = (0.8 + 0.01 * xx + 0.02 * yy + 0.05 * np.sin(0.9 * xx) * np.cos(0.7 * yy) + rng.uniform(0, 0.01, (H, W))).astype(np.float32)
    d[H // 2:H // 2 + 4, 2:8] = np.float32(1.25)       # constant depth
    d[1, 3] = d[2, 3] = d[H - 3, W - 2] = 0            # holes
    d[3, W // 2] = np.float32(cutoff)                  # at the cutoff: invalid
    d[4, W // 2 + 1] = np.float32(cutoff) + 3          # above it
    d[H // 2 + 1, W - 4] = np.nan
    d[0, 0] = np.float32(cutoff) - np.float32(1e-3)    # just below it: valid
    return d


def main(reference_root):
    rng = np.random.default_rng(30101)
    arrays, names = {}, []
    with tempfile.TemporaryDirectory() as tmp:
        exe = build(reference_root, tmp)
        for name, H, W, intr, cutoff in (("frame_12x20", 12, 20, (1066.778, 1067.487, 6.3, 9.9), 20.0),
                                         ("frame_19x37", 19, 37, (572.4114, 573.57043, 9.0, 18.25), 2.0)):
            intr = np.array(intr, np.float32)
            depth = frame(rng, H, W, cutoff)
            nmap = run(exe, tmp, depth, intr, cutoff)
            assert np.isnan(nmap[-1]).all() and np.isnan(nmap[:, -1]).all() and np.isfinite(nmap).any()
            names.append(name)
            arrays["%s/depth" % name] = depth
            arrays["%s/intrinsics" % name] = intr
            arrays["%s/cutoff" % name] = np.float32(cutoff)
            arrays["%s/nmap" % name] = nmap
    arrays["names"] = np.array(names)
    path = os.path.join(HERE, "normals.npz")
    np.savez_compressed(path, **arrays)
    print("%s: %d frames, %d bytes" % (path, len(names), os.path.getsize(path)))


if __name__ == "__main__":
    root = sys.argv[1] if len(sys.argv) == 2 else os.environ.get("POSECNN_REFERENCE")
    if not root:
        sys.exit(__doc__)
    main(root)
