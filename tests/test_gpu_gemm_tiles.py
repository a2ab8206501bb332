"""GPU: the 256 x 256 encoder GEMM kernels (csrc/kernels_gemm.hip: gemm_bf16_v3_kernel and the persistent kernel in its plain
"v4" and tail-re-tiled "v5" forms) are compositions of ONE tile body, so their agreeing with each other no longer says much.
This test also pins the bits: CRC32s of the encoder output and of every cross-KV block, recorded on the commit BEFORE the kernels
were merged into one body (tests/golden/gemm_tiles_crc.json names it), must come out unchanged.

One encode of 6 clips at large-v3 width (2 + 2 layers, M = 9 000 rows = 36 m-tiles with a clamped last tile) reaches every path
on 256 CUs:
  qkv        540 tiles  persistent, workgroups walk up to three tiles (carried stores), 128-row tail tiles ("v5")
  fc1        720 tiles  persistent, no tail plan fits ("v4")
  out / fc2  180 tiles  one workgroup per tile (v3)
  cross-KV   2 x 360    one grouped persistent launch over both layers (xkv_grouped = 1) or v3 per layer (= 0)
The 192-row tail tiles are covered by test_gpu_parity.test_round4_options_are_bit_identical_to_their_off_form (16 clips)."""
import json
import os
import zlib

import numpy as np
import pytest

from taiwan_tongues_asr_ce_amd import synth
from taiwan_tongues_asr_ce_amd.config import COMPUTE_BF16, COMPUTE_F16, PRESETS

pytestmark = pytest.mark.gpu
B = 6
COMPUTE = {"bf16": COMPUTE_BF16, "f16": COMPUTE_F16}
BLOCKS = ("encoder", "xkv_l0_k", "xkv_l0_v", "xkv_l1_k", "xkv_l1_v")


def run_all_forms(dtype):
    """{(enc_gemm, xkv_grouped): [encoder output, 4 cross-KV blocks]} and the kernel signatures of the automatic choice."""
    from taiwan_tongues_asr_ce_amd.engine import Engine
    dims = PRESETS["large-v3-w2"]
    e = Engine(dims, COMPUTE[dtype], B)
    e.load_weights(synth.iter_weights(dims))
    e.log_mel([synth.noise_clip(70 + i) if i % 2 else synth.tonal_clip(70 + i) for i in range(B)], want_output=False)
    outs = {}
    for enc_gemm in (0, 3, 4):
        for grouped in (1, 0):
            e.set_option("enc_gemm", enc_gemm)
            e.set_option("xkv_grouped", grouped)
            enc = e.encode(B, want_output=True)
            outs[(enc_gemm, grouped)] = [enc] + [e.cross_kv(layer, which, B) for layer in (0, 1) for which in (0, 1)]
    e.set_option("enc_gemm", 0)
    e.set_option("xkv_grouped", 1)
    sigs = {n: e.bench_kernel(n, B, iters=1)["signature"] for n in ("enc_gemm_qkv", "enc_gemm_fc1", "enc_gemm_out")}
    e.close()
    return outs, sigs


def crcs(blocks):
    return {name: zlib.crc32(np.ascontiguousarray(a).tobytes()) for name, a in zip(BLOCKS, blocks)}


@pytest.mark.parametrize("dtype", ["bf16", "f16"])
def test_every_tile_form_gives_the_bits_of_the_separate_kernels(golden_dir, dtype):
    outs, sigs = run_all_forms(dtype)
    print(sigs)
    # the batch must keep reaching each form (another CU count: change B, not these)
    assert sigs["enc_gemm_qkv"].startswith("gemm_bf16_v5_kernel<"), sigs
    assert sigs["enc_gemm_fc1"].startswith("gemm_bf16_v4_kernel<"), sigs
    assert sigs["enc_gemm_out"].startswith("gemm_bf16_v3_kernel<"), sigs
    ref = outs[(0, 1)]
    for key, cur in outs.items():
        for name, a, b in zip(BLOCKS, cur, ref):
            assert np.array_equal(a, b), (key, name)
    with open(os.path.join(golden_dir, "gemm_tiles_crc.json")) as f:
        want = json.load(f)[dtype]
    got = crcs(ref)
    print(got)
    assert got == want
