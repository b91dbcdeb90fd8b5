"""HIP/CDNA4 GPU health kernels (native/gpu/hip/: hbm.hip, mfma.hip, lds.hip, cache.hip, valu.hip, atomic.hip, regfile.hip, xlane.hip, gemm_soak.hip) exposed to Python.

These are the only compute kernels in the framework: the reference controller has none
(SURVEY §2.5).  They back the node agent's diagnostics before a GPU is advertised
(native/gpu/diag_runner.cc) and can be run by hand:

* ``hbm(device)``       — HBM3E pattern fill / copy / verify at streaming bandwidth
* ``hbm_walk(device)``  — address-in-data walk over most of the free HBM (stuck bits,
  aliased addresses), reporting the first bad address
* ``mfma(device)``      — exact-integer bf16 MFMA tiles on every CU + a throughput pass
* ``mfma_lowp(device)`` — the same for the MX block-scaled fp8 / fp4 matrix-core path
  (``v_mfma_scale_f32_16x16x128_f8f6f4``), with and without E8M0 block scales
* ``mfma_classic(device)`` — the same for the fp16, int8, fp32-input and fp64 matrix-core paths, with
  operands as wide as each path's multipliers
* ``lds(device)``       — a march test of every CU's whole Local Data Share (160 KiB), attributed to
  the CU, then the aggregate LDS read rate
* ``cache(device)``     — a march through every XCD's L2 (4 MiB each), attributed to the XCC, and the
  aggregate L2 read rate; then a pattern check and the read rate of the 256 MiB Infinity Cache
* ``valu(device)``      — the vector ALU's integer, fp32, fp16, fp64, conversion, integer-dot and transcendental
  instructions on every SIMD, refereed by the host CPU and attributed to CU, SIMD and lane; then the vector rates
* ``atomic(device)``    — every global and LDS atomic form (integer, 64-bit, fp32, fp64, packed bf16 / fp16 adds, compare-and-swap,
  returning adds as tickets) in a table per workgroup and in one shared by the launch, refereed by the host CPU; then the atomic rates
* ``regfile(device)``   — a march of every SIMD's whole vector register file (512 registers a lane, 128 KiB a SIMD) in two
  layouts, attributed to CU, SIMD, register and lane; then a rotate of 504 registers, a moving-data check and the move rate
* ``xlane(device)``     — the cross-lane paths (DPP, the half-wave swaps, the LDS crossbar's permutes, the moves between lanes
  and scalar registers) on every SIMD, refereed by the host CPU and attributed to CU, SIMD and lane; then the cross-lane rates
* ``gemm_check(device)``— a bf16 GEMM on the matrix cores checked element by element against
  a double-precision product of the same operands on the host
* ``gemm_soak(device)`` — the sustained-throughput soak: the 8-phase ping-pong GEMM
  (256x256 tiles) for ``launches`` launches, every result checksummed
* ``gemm(a, b)``       — the one-wave-per-tile MFMA GEMM on caller operands (A: MxK, B: KxN bf16),
  fp32 result; the plainest use of the bf16 operand layout, for comparison with the others
* ``gemm_tiled(a, bt)`` — the soak's kernel on caller operands (A: MxK, Bt: NxK bf16),
  fp32 result; used to check the kernel against a PyTorch fp32 product
* ``mx_gemm(a, sa, bt, sbt, fmt)`` — the MX block-scaled matrix-core path on caller
  codes (fp8 e4m3 bytes or packed fp4 e2m1) and E8M0 scales; used to check the hardware's
  operand/scale layout against an independent PyTorch decode
* ``pcie(device)``      — host<->device copy bandwidth, pinned
* ``device_bdf(device)``— the HIP device's PCI address, to match it to amdsmi / kubelet
* ``hbm_planted``, ``hbm_walk_planted``, ``pcie_planted``, ``mfma_planted``,
  ``mfma_lowp_planted``, ``mfma_classic_planted``, ``lds_planted``, ``cache_planted``, ``valu_planted``, ``atomic_planted``, ``regfile_planted``, ``xlane_planted``, ``gemm_soak_planted``, ``burn_planted`` — for tests: the same diagnostics with wrong
  values planted in their own data, to show that they are detected (see below)
* ``mfma_delayed``, ``burn_delayed``, ``cache_delayed``, ``valu_delayed``, ``atomic_delayed``, ``regfile_delayed``, ``xlane_delayed`` — for tests: the matrix-core throughput, the burn, the L2 rate, the vector and the atomic rates with
  chosen waves, launches or workgroups made slow by a known time, to show that it reaches the rates
* ``hbm_data``, ``hbm_walk_data``, ``pcie_data``, ``gemm_soak_data``, ``mfma_tile``, ``mfma_classic_tile``, ``lds_data``, ``cache_data``, ``valu_data``, ``valu_expected``, ``atomic_data``, ``atomic_expected``, ``atomic_rate_expected``, ``regfile_data``, ``regfile_expected``, ``regfile_layout``, ``xlane_data``, ``xlane_expected`` — for tests:
  the same diagnostics, returning the data they generated for themselves (see below)

All fail loudly (RuntimeError) if ``libbgc_gpu_diag.so`` or the GPU is missing; there
is no CPU fallback.
"""
import json

import numpy as np

from .. import native


def library_path():
    return native().diag_library_path()


def device_count():
    return native().diag_device_count()


def device_arch(device=0):
    return native().diag_device_arch(device)


def device_bdf(device=0):
    return native().diag_device_bdf(device)


def hbm(device=0, nbytes=2 << 30, iters=3, seed=0x5EED):
    return json.loads(native().diag_hbm(device, nbytes, iters, seed))


def hbm_walk(device=0, fraction=0.9, chunk_bytes=4 << 30, budget_ms=20000, seed=0x5EED):
    return json.loads(native().diag_hbm_walk(device, fraction, chunk_bytes, budget_ms, seed))


def mfma(device=0, waves_per_cu=32, iters=4096, seed=0x5EED):
    return json.loads(native().diag_mfma(device, waves_per_cu, iters, seed))


def mfma_lowp(device=0, waves_per_cu=32, iters=4096, seed=0x5EED):
    """MX block-scaled fp8 (e4m3) and fp4 (e2m1) matrix-core tiles on every CU, with unit
    and random E8M0 block scales, checked exactly; then the dense fp8 and fp4 rates."""
    return json.loads(native().diag_mfma_lowp(device, waves_per_cu, iters, seed))


CLASSIC_PATHS = {"fp16": 0, "int8": 1, "fp32": 2, "fp64": 3}  # BGC_CLASSIC_*: the order of every per-path list
CLASSIC_K = {"fp16": 32, "int8": 64, "fp32": 4, "fp64": 4}
CLASSIC_DTYPES = {"fp16": np.float16, "int8": np.int8, "fp32": np.float32, "fp64": np.float64}
CLASSIC_CHECK_ROUNDS = 4  # BGC_CLASSIC_CHECK_ROUNDS


def _classic_path(path):
    """a path's name, or its number as it is (so a test can pass one out of range)"""
    return CLASSIC_PATHS.get(path, path) if isinstance(path, str) else path


def mfma_classic(device=0, waves_per_cu=32, iters=8192, seed=0x5EED):
    """The fp16, int8, fp32-input and fp64 matrix cores: exact tiles with full-width operands on every
    CU, then each path's dense rate (``fp16_tflops``, ``int8_tops``, ``fp32_tflops``, ``fp64_tflops``;
    ``rate_ms`` in that order)."""
    return json.loads(native().diag_mfma_classic(device, waves_per_cu, iters, seed))


def lds(device=0, wgs_per_cu=4, rate_iters=8192, seed=0x5EED):
    """Every CU's Local Data Share: `wgs_per_cu` workgroups per CU each write and verify all 160 KiB
    twice (a hash pattern, then its inverse), binned by the CU they ran on; then `rate_iters`
    sweeps of 16-byte reads over the array on every CU for the aggregate read rate."""
    return json.loads(native().diag_lds(device, wgs_per_cu, rate_iters, seed))


L2_REGION_BYTES = 96 << 10  # BGC_L2_REGION_BYTES: 32 workgroups of an XCD hold 3 MiB of its 4 MiB L2
L2_SLAB_BYTES = 32 << 10  # a region is 1..4 of these
# Sweep counts that put each timed launch of cache() at 2-4 ms on the MI355X (tools/probes/cache_rate_probe.py,
# profiles/cache_diag/cache_rates.json, 12 runs each right after an MFMA check): 4096 sweeps of 96 KiB regions take
# 3.27-3.44 ms at 30.0-31.6 TB/s, and 128 sweeps of 128 MiB take 2.22-2.51 ms at 6.8-7.7 TB/s.  The whole run is
# 5.9-6.1 ms of kernels, 6.6-6.8 ms with its allocations.
L2_SWEEPS = 4096
IC_BYTES = 128 << 20
IC_SWEEPS = 128


def cache(device=0, rounds=4, region_bytes=L2_REGION_BYTES, l2_sweeps=L2_SWEEPS, ic_bytes=IC_BYTES, ic_sweeps=IC_SWEEPS,
          seed=0x5EED):
    """The two SRAM levels between the LDS and HBM.  L2: one workgroup per CU writes and verifies a
    region of `region_bytes` (32, 64, 96 or 128 KiB) twice per round (a hash pattern, then its
    inverse) through the L2 of the XCD it runs on, for `rounds` rotations of the regions, binned by
    XCC; then `l2_sweeps` L1-bypassing sweeps of every region for the aggregate L2 read rate.
    Infinity Cache (`ic_bytes` 0 turns it off): a buffer of `ic_bytes` is filled, checked word by
    word, swept `ic_sweeps` times under a 32-bit sum, and checked again."""
    return json.loads(native().diag_cache(device, rounds, region_bytes, l2_sweeps, ic_bytes, ic_sweeps, seed))


VALU_CLASSES = ("int32", "fp32", "fp16", "fp64", "cvt", "dot", "trans")  # BGC_VALU_*: the order of class_mismatches
VALU_CLASS_WORDS = (13, 6, 3, 6, 5, 2, 5)  # 32-bit result words of a class per round, 40 in all (BGC_VALU_ROUND_WORDS)
VALU_ROUND_WORDS = 40
VALU_RATE_CLASSES = ("fp32", "fp16", "fp64", "int32", "trans")  # BGC_VALU_RATE_*: the order of rate_ms
# Defaults of valu(), from tools/probes/valu_rate_probe.py on the MI355X (profiles/valu_diag/rates.json, 12 runs per point, each
# right after an MFMA check).  The rates rise with the iterations until the launch outlasts its ramp: at 2 waves per SIMD, fp32
# reads 102-106 TF/s at 1024 iterations, 112-117 at 4096 and 115-120 at 16384, where the five timed launches take 0.53-0.59 ms
# each (trans 1.4 ms).  The whole run is then 3.7-4.2 ms of kernels, 9.1-9.3 ms with its copies and the host referee (14 ms in
# a fresh process).  More waves per SIMD read more (8: 128-130 TF/s fp32) at 4 times the time and the digests to copy.
VALU_WAVES_PER_SIMD = 2
VALU_ROUNDS = 16
VALU_RATE_ITERS = 16384


def _valu_code(names, name):
    """a class's name, or its number as it is (so a test can pass one out of range)"""
    return names.index(name) if isinstance(name, str) else name


def valu(device=0, waves_per_simd=VALU_WAVES_PER_SIMD, rounds=VALU_ROUNDS, rate_iters=VALU_RATE_ITERS, seed=0x5EED):
    """The vector ALU: cus * `waves_per_simd` (1..8) workgroups of four waves each run `rounds` (1..64) rounds of a
    fixed instruction sequence in seven classes (VALU_CLASSES) on per-lane operands and write a digest per lane and
    class; the host CPU recomputes the six exact classes, judges the transcendentals by the waves' consensus and
    against libm, and names the CU, SIMD and lane of a wrong value.  Then each rate class (VALU_RATE_CLASSES) runs
    `rate_iters` (1..65536) iterations of 8 chains per lane: ``fp32_tflops``, ``fp16_tflops``, ``fp64_tflops``,
    ``int32_tops``, ``trans_tips`` (10^12 v_exp_f32 per second); ``rate_ms`` in that order."""
    return json.loads(native().diag_valu(device, waves_per_simd, rounds, rate_iters, seed))


def valu_trans_ulps():
    """The accuracy bounds of v_exp_f32, v_log_f32, v_rcp_f32, v_rsq_f32 and v_sqrt_f32 against double-precision
    libm, in units of the last place of the fp32 result (BGC_VALU_*_ULPS)."""
    return tuple(native().diag_valu_trans_ulps())


ATOMIC_PLACEMENTS = ("own", "shared")  # BGC_ATOMIC_OWN, _SHARED
ATOMIC_CLASSES = ("int32", "int64", "f32", "f64", "pk16", "cas", "ticket", "lds")  # BGC_ATOMIC_*: the order of own_mismatches
ATOMIC_CLASS_WORDS = (6, 2, 1, 2, 2, 1, 1, 9)  # 32-bit words of a class's element
ATOMIC_CLASS_OPS = (6, 1, 1, 1, 2, 1, 1, 9)  # the words a plant can name
ATOMIC_INT_WORDS = ("add", "smin", "umax", "and", "or", "xor")
ATOMIC_LDS_WORDS = ("add", "ticket", "umax", "smin", "and", "or", "xor", "add_f32", "cas")
ATOMIC_RATE_CLASSES = ("f32", "pk_bf16", "u32", "rtn")  # BGC_ATOMIC_RATE_*: the order of rate_ms
ATOMIC_EMPTY = 0xFFFFFFFF
# Defaults of atomic(), from tools/probes/atomic_rate_probe.py on the MI355X (profiles/atomic_diag/rates.json, 12 runs per point, each
# right after an MFMA check).  rate_iters is odd, so that the float rows do not all end at 0: 4095 visits row 63 an odd number of times.
# The rates rise with the iterations until the launch outlasts its ramp: the fp32 add reads 1.24-1.27 TB/s at 1023 iterations, 1.33-1.34
# at 4095 and 1.35-1.36 at 16383, where the returning adds alone take 39 ms.  The run is 14.5 ms of kernels, 0.25 ms of them the check, and
# 133-135 ms with its copies and the host referee, whose time follows the check's size: about 60 ms per workgroup per CU.
ATOMIC_WGS_PER_CU = 2
ATOMIC_ROUNDS = 8
ATOMIC_RATE_ITERS = 4095


def atomic(device=0, wgs_per_cu=ATOMIC_WGS_PER_CU, rounds=ATOMIC_ROUNDS, rate_iters=ATOMIC_RATE_ITERS, seed=0x5EED):
    """Atomic read-modify-writes: cus * `wgs_per_cu` (1..8) workgroups of four waves each run `rounds` (1..64) rounds of every
    class (ATOMIC_CLASSES) on hashed operands, in a table of the workgroup's own (``own_mismatches``; a wrong element names the
    CU) and in one shared by the launch (``shared_mismatches``).  Every final value is independent of the order of arrival; the
    host CPU recomputes the tables and checks every compare-and-swap and every ticket by its property.  Then each rate class
    (ATOMIC_RATE_CLASSES) runs `rate_iters` (1..65536) iterations: ``f32_add_tbps``, ``pk_bf16_add_tbps``, ``u32_add_tbps``
    (TB/s of added bytes), ``rtn_gops`` (10^9 returning adds per second); ``rate_ms`` in that order."""
    return json.loads(native().diag_atomic(device, wgs_per_cu, rounds, rate_iters, seed))


REGFILE_REGS = 512  # of a lane: v0..v255 are 0..255, a0..a255 are 256..511
REGFILE_PHASES = ("layout0_pass0", "layout0_pass1", "layout1_pass0", "layout1_pass1", "rotate")  # a plant's or a dump's phase, 0..4
REGFILE_ROTATE = 4
REGFILE_PLANT_REGS = (0, 5, 128, 250, 255, 256, 384, 511)  # BGC_REGFILE_PLANT_REGS: the register of a plant's slot
# Defaults of regfile(): every SIMD is marched twice, by waves of different seeds, and the rotate runs long enough for
# the launch to outlast its ramp (profiles/regfile_diag/rates.json).
REGFILE_WGS_PER_CU = 2
REGFILE_SWEEPS = 4096


def regfile(device=0, wgs_per_cu=REGFILE_WGS_PER_CU, sweeps=REGFILE_SWEEPS, seed=0x5EED):
    """The vector register file as a memory: cus * `wgs_per_cu` (1..8) workgroups whose four waves each hold a SIMD's whole file
    (512 registers a lane) march it with a per-wave pattern and its inverse in two layouts that together cover every register
    (``vgpr_mismatches``, ``agpr_mismatches``), then rotate a ring of 504 registers by one place `sweeps` (1..65536) times and
    verify where every word arrived (``rotate_mismatches``, ``rate_ok``): ``mov_tops`` is 10^12 lane-moves per second.  A wrong
    word names its CU, SIMD, register (``first_bad_reg`` 0..511, ``first_bad_reg_name``), lane and phase."""
    return json.loads(native().diag_regfile(device, wgs_per_cu, sweeps, seed))


XLANE_CLASSES = ("row", "wave", "mask", "alu", "swap", "lds", "lane", "exec")  # BGC_XLANE_*: the order of class_mismatches
XLANE_CLASS_WORDS = (12, 6, 6, 3, 4, 6, 6, 4)  # 32-bit result words of a class per round, 47 in all (BGC_XLANE_ROUND_WORDS)
XLANE_ROUND_WORDS = 47
XLANE_RATE_CLASSES = ("dpp", "swap", "bpermute", "swizzle")  # BGC_XLANE_RATE_*: the order of rate_ms
# Defaults of xlane(), from tools/probes/xlane_rate_probe.py on the MI355X (profiles/xlane_diag/rates.json, 12 runs per point, each
# right after an MFMA check).  Every SIMD is checked by two waves.  The rates rise with the iterations until the launch outlasts its
# ramp: at 2 waves per SIMD the DPP move reads 27.9-29.0 x 10^12 lane-moves per second at 1024 iterations, 31.7-32.3 at 4096 and
# 32.8-33.7 at 16384, where the run is 4.7 ms of kernels (2.7 ms of them the ds_bpermute launch) and 6.2 ms with its copies and the
# host referee.  8 waves per SIMD read more (35.4-36.3) at 4 times the time.
XLANE_WAVES_PER_SIMD = 2
XLANE_ROUNDS = 16
XLANE_RATE_ITERS = 16384


def xlane(device=0, waves_per_simd=XLANE_WAVES_PER_SIMD, rounds=XLANE_ROUNDS, rate_iters=XLANE_RATE_ITERS, seed=0x5EED):
    """The cross-lane paths: cus * `waves_per_simd` (1..8) workgroups of four waves each run `rounds` (1..64) rounds of a
    fixed sequence of DPP moves and arithmetic, half-wave swaps, ds_bpermute / ds_permute / ds_swizzle, v_readlane,
    v_readfirstlane, v_writelane, ballots and moves under a partial EXEC mask in eight classes (XLANE_CLASSES) on hashed
    operands and write a digest per lane and class; the host CPU recomputes every digest and names the CU, SIMD and
    destination lane of a wrong value.  Then each rate class (XLANE_RATE_CLASSES) runs `rate_iters` (1..65536) steps of
    8 chains per lane: ``dpp_tops``, ``swap_tops``, ``bpermute_tops``, ``swizzle_tops`` (10^12 lane-moves per second);
    ``rate_ms`` in that order."""
    return json.loads(native().diag_xlane(device, waves_per_simd, rounds, rate_iters, seed))


def gemm_check(device=0, m=4096, n=4096, k=4096, seed=0x5EED):
    return json.loads(native().diag_gemm_check(device, m, n, k, seed))


def gemm_soak(device=0, m=8192, n=8192, k=8192, launches=10, seed=0x5EED):
    return json.loads(native().diag_gemm_soak(device, m, n, k, launches, seed))


def pcie(device=0, nbytes=256 << 20, iters=5, seed=0x5EED):
    return json.loads(native().diag_pcie(device, nbytes, iters, seed))


# ---------------------------------------------------------------------------------------------
# Planted variants, for tests only: the same diagnostics with deliberately wrong values written
# into their own buffers or accumulators between the phase that produces the data and the phase
# that checks it, to show that a wrong value reaches the counters.  Plants are lists of tuples; an
# empty list is the production run.  A plant outside the buffer (or a wave, lane, round or index out
# of range) is refused with "invalid arguments" before the GPU is touched.  Neither the node agent
# nor judge can ask for a plant.

ALL_WAVES = -1  # `wave` of a check-phase plant: every wave

_LOWP_VARIANTS = {"fp8": 0, "fp8_scaled": 1, "fp4": 2, "fp4_scaled": 3}
_LOWP_FORMATS = {"fp8": 0, "fp4": 1}


def hbm_planted(nbytes, plants, device=0, seed=0x5EED):
    """One fill, copy and check with `plants` = [(32-bit word index, xor mask), ...] applied to
    the copy before the check.  The rates are those of one cold iteration: no measurement."""
    return json.loads(native().diag_hbm_planted(device, nbytes, seed, list(plants)))


def hbm_walk_planted(nbytes, chunk_bytes, plants, device=0, seed=0x5EED):
    """The walk over `nbytes` in chunks of `chunk_bytes` with `plants` = [(pass, chunk, 64-bit
    word offset in the chunk, xor mask), ...] applied after that pass's fill.  The result also
    lists the chunks as ``chunk_list`` = [[device address, bytes], ...]."""
    return json.loads(native().diag_hbm_walk_planted(device, nbytes, chunk_bytes, seed, list(plants)))


def pcie_planted(nbytes, plants, device=0, seed=0x5EED):
    """The round trip with `plants` = [(64-bit word index, xor mask), ...] applied to the device
    buffer between the upload and the copies back."""
    return json.loads(native().diag_pcie_planted(device, nbytes, seed, list(plants)))


def mfma_planted(check_plants, rate_plants=(), device=0, waves_per_cu=1, iters=64, seed=0x5EED):
    """`check_plants` = [(wave or ALL_WAVES, round, lane, i, delta), ...] add delta to acc[i] of
    that lane before the comparison; `rate_plants` = [(wave, lane, chain, i, delta), ...] do so
    after the throughput loop."""
    return json.loads(native().diag_mfma_planted(device, waves_per_cu, iters, seed, list(check_plants), list(rate_plants)))


def mfma_lowp_planted(check_plants, rate_plants=(), device=0, waves_per_cu=1, iters=64, seed=0x5EED):
    """As mfma_planted, with the variant ("fp8", "fp8_scaled", "fp4", "fp4_scaled") in front of a
    check plant and the format ("fp8", "fp4") in front of a rate plant."""
    check = [(_LOWP_VARIANTS[p[0]],) + tuple(p[1:]) for p in check_plants]
    rate = [(_LOWP_FORMATS[p[0]],) + tuple(p[1:]) for p in rate_plants]
    return json.loads(native().diag_mfma_lowp_planted(device, waves_per_cu, iters, seed, check, rate))


def mfma_classic_planted(check_plants, rate_plants=(), device=0, waves_per_cu=1, iters=64, seed=0x5EED):
    """As mfma_planted, with the path ("fp16", "int8", "fp32", "fp64", or its number) in front of
    every plant.  The delta is converted to the path's accumulator type; an int8 delta must be an
    integer below 2^31 in magnitude."""
    check = [(_classic_path(p[0]),) + tuple(p[1:]) for p in check_plants]
    rate = [(_classic_path(p[0]),) + tuple(p[1:]) for p in rate_plants]
    return json.loads(native().diag_mfma_classic_planted(device, waves_per_cu, iters, seed, check, rate))


LDS_WORDS = 40960  # 32-bit words of a CU's Local Data Share


def lds_planted(plants, device=0, wgs_per_cu=1, rate_iters=64, seed=0x5EED):
    """`plants` = [(workgroup or ALL_WAVES, pass, word, xor mask), ...]: thread 0 of that march
    workgroup XORs the mask into that word of its LDS after the pass's fill and before its verify.
    The rate phase takes no plant."""
    return json.loads(native().diag_lds_planted(device, wgs_per_cu, rate_iters, seed, list(plants)))


def cache_planted(l2_plants, ic_plants=(), device=0, rounds=1, region_bytes=L2_REGION_BYTES, l2_sweeps=16, ic_bytes=2 << 20,
                  ic_sweeps=2, seed=0x5EED):
    """`l2_plants` = [(round, workgroup or ALL_WAVES, pass, word of the region, xor mask), ...]: thread 0
    of that march workgroup XORs the mask into that word with a plain store after the pass's fill
    and before its verify.  `ic_plants` = [(when, word of the buffer, xor mask), ...]: applied from
    the host after the fill (when 0: both checks and the sweeps' sum see it) or after the timed
    sweeps (when 1: the last check alone)."""
    return json.loads(native().diag_cache_planted(device, rounds, region_bytes, l2_sweeps, ic_bytes, ic_sweeps, seed,
                                                  list(l2_plants), list(ic_plants)))


def valu_planted(check_plants, rate_plants=(), device=0, waves_per_simd=1, rounds=2, rate_iters=16, seed=0x5EED):
    """`check_plants` = [(wave or ALL_WAVES, class, round, lane, result word of the class, xor mask), ...]: that wave
    XORs the mask into that result word before it folds it into the digest.  `rate_plants` = [(wave or ALL_WAVES,
    rate class, lane, chain, xor mask), ...] do so to the first word of that chain after the loop of that class's
    timed launch.  Classes by name (VALU_CLASSES, VALU_RATE_CLASSES) or number."""
    check = [(p[0], _valu_code(VALU_CLASSES, p[1])) + tuple(p[2:]) for p in check_plants]
    rate = [(p[0], _valu_code(VALU_RATE_CLASSES, p[1])) + tuple(p[2:]) for p in rate_plants]
    return json.loads(native().diag_valu_planted(device, waves_per_simd, rounds, rate_iters, seed, check, rate))


def xlane_planted(check_plants, rate_plants=(), device=0, waves_per_simd=1, rounds=2, rate_iters=16, seed=0x5EED):
    """xlane() with check plants (wave or -1 for every wave, class, round, destination lane, result word of the class, xor
    mask), applied to the word before it is folded into the digest, and rate plants (wave or -1, rate class, lane, chain
    0..7, xor mask), applied to the chain's end value after the loop of that class's timed launch.  Classes by name
    (XLANE_CLASSES, XLANE_RATE_CLASSES) or number."""
    check = [(p[0], _valu_code(XLANE_CLASSES, p[1])) + tuple(p[2:]) for p in check_plants]
    rate = [(p[0], _valu_code(XLANE_RATE_CLASSES, p[1])) + tuple(p[2:]) for p in rate_plants]
    return json.loads(native().diag_xlane_planted(device, waves_per_simd, rounds, rate_iters, seed, check, rate))


def _atomic_plants(plants):
    """(placement, class, word, wave, round, lane, times, mask) with the placement and the class by name or number"""
    return [(_valu_code(ATOMIC_PLACEMENTS, p[0]), _valu_code(ATOMIC_CLASSES, p[1])) + tuple(p[2:]) for p in plants]


def _atomic_rate_plants(plants):
    return [(_valu_code(ATOMIC_RATE_CLASSES, p[0]),) + tuple(p[1:]) for p in plants]


def atomic_planted(plants, rate_plants=(), device=0, wgs_per_cu=1, rounds=2, rate_iters=15, seed=0x5EED):
    """`plants` = [(placement, class, word of the element, wave, round, lane, times, xor mask), ...]: that lane issues that
    atomic `times` (0..2) times, its operand word XORed with the mask.  `rate_plants` = [(rate class, wave, lane, times), ...]:
    that lane issues the atomic of the last iteration of that class's timed launch `times` (0 or 2) times."""
    return json.loads(native().diag_atomic_planted(device, wgs_per_cu, rounds, rate_iters, seed, _atomic_plants(plants),
                                                   _atomic_rate_plants(rate_plants)))


def atomic_delayed(delays, device=0, wgs_per_cu=1, rounds=2, rate_iters=15, seed=0x5EED):
    """`delays` = [(rate class, wave or ALL_WAVES, ticks), ...]: in that class's timed rate launch that wave waits `ticks` of the
    100 MHz constant clock after its loop and before it reads its end time.  No value is touched."""
    return json.loads(native().diag_atomic_delayed(device, wgs_per_cu, rounds, rate_iters, seed, _atomic_rate_plants(delays)))


MAX_DELAY_TICKS = 10_000_000  # 100 ms of the 100 MHz constant clock


def regfile_planted(plants, device=0, wgs_per_cu=1, sweeps=3, seed=0x5EED):
    """`plants` = [(wave or ALL_WAVES, phase 0..4, slot of REGFILE_PLANT_REGS, lane, xor mask), ...]: that register of that lane
    is XORed with the mask after the fill of that phase and before its verify; in the rotate (phase 4) before the sweeps.  The
    phase must hold a pattern in the register: a layout's own eight (``regfile_layout()``) are refused."""
    return json.loads(native().diag_regfile_planted(device, wgs_per_cu, sweeps, seed, [tuple(p) for p in plants]))


def regfile_delayed(delays, device=0, wgs_per_cu=1, sweeps=64, seed=0x5EED):
    """`delays` = [(wave or ALL_WAVES, ticks), ...]: in the timed rotate launch that wave waits `ticks` of the 100 MHz constant
    clock after its loop and before it reads its end time.  No value is touched; the time shows in mov_tops, rotate_ms,
    slowest_cu_key, slowest_simd and simd_balance."""
    return json.loads(native().diag_regfile_delayed(device, wgs_per_cu, sweeps, seed, [tuple(d) for d in delays]))


def xlane_delayed(delays, device=0, waves_per_simd=1, rounds=2, rate_iters=16, seed=0x5EED):
    """xlane() with (wave or -1, rate class, ticks): that wave of that class's timed launch waits `ticks` of the 100 MHz
    constant clock after its loop and before it reads its end time.  No value is touched; the time shows in the class's
    rate, rate_ms, slowest_cu_key and cu_balance."""
    return json.loads(native().diag_xlane_delayed(device, waves_per_simd, rounds, rate_iters, seed,
                                                  [(d[0], _valu_code(XLANE_RATE_CLASSES, d[1]), d[2]) for d in delays]))


def valu_delayed(delays, device=0, waves_per_simd=1, rounds=2, rate_iters=16, seed=0x5EED):
    """`delays` = [(wave or ALL_WAVES, rate class, ticks), ...]: in that class's timed rate launch that wave waits
    `ticks` of the 100 MHz constant clock after its loop and before it reads its end time.  No value is touched;
    the time shows in the class's rate and rate_ms, in slowest_cu_key and in cu_balance."""
    return json.loads(native().diag_valu_delayed(device, waves_per_simd, rounds, rate_iters, seed,
                                                 [(d[0], _valu_code(VALU_RATE_CLASSES, d[1]), d[2]) for d in delays]))


def cache_delayed(delays, device=0, rounds=1, region_bytes=L2_REGION_BYTES, l2_sweeps=16, ic_bytes=2 << 20, ic_sweeps=2,
                  seed=0x5EED):
    """`delays` = [(workgroup or ALL_WAVES, ticks), ...]: in the timed L2 rate launch that workgroup
    waits `ticks` of the 100 MHz constant clock after its loop and before it reads its end time.  No
    value is touched; the time shows in l2_read_tbps, xcc_us, slowest_xcc and xcc_balance."""
    return json.loads(native().diag_cache_delayed(device, rounds, region_bytes, l2_sweeps, ic_bytes, ic_sweeps, seed, list(delays)))


def mfma_delayed(delays, device=0, waves_per_cu=1, iters=64, seed=0x5EED):
    """`delays` = [(wave or ALL_WAVES, ticks), ...]: in the timed throughput launch that wave waits,
    after its loop and before its comparison, until `ticks` of the 100 MHz constant clock have
    passed.  Its values are untouched; its time shows in tflops, xcc_wave_us and xcc_balance."""
    return json.loads(native().diag_mfma_delayed(device, waves_per_cu, iters, seed, list(delays)))


def burn_delayed(duration_ms, first_delayed_launch, ticks, dtype="bf16", device=0, waves_per_cu=32, seed=0x5EED):
    """The burn's loop (without the telemetry that ``diag_burn`` adds) with every wave of launch
    `first_delayed_launch` (0-based) and of every later one delayed by `ticks`."""
    return json.loads(native().diag_burn_delayed(device, duration_ms, waves_per_cu, seed, dtype, first_delayed_launch, ticks))


def burn_planted(duration_ms, plants, dtype="bf16", device=0, waves_per_cu=32, seed=0x5EED):
    """The burn's loop with `plants` = [(launch, wave, lane, chain, i, delta), ...]: launch `launch`
    (0-based) adds delta to acc[chain][i] of that lane after its loop and before its comparison.  The
    first launch runs 2048 iterations, the later ones the retuned length; a launch the burn never
    reaches has no effect."""
    return json.loads(native().diag_burn_planted(device, duration_ms, waves_per_cu, seed, dtype, list(plants)))


def gemm_soak_planted(m, n, k, launches, plants, device=0, seed=0x5EED):
    """`plants` = [(launch, row, col, delta), ...] add delta to C[row][col] after that launch and
    before its checksums; only the first and the last launch are checked."""
    return json.loads(native().diag_gemm_soak_planted(device, m, n, k, launches, seed, list(plants)))


# ---------------------------------------------------------------------------------------------
# Generated data, for tests only: the same diagnostics, returning the data they generated for
# themselves (gpu_diag.h documents every pattern) next to their result, so a test can compare it
# with an independent reference.  At most 128 MiB come back from one call.

TILE_PATHS = {"bf16": 0, "fp8": 1, "fp4": 2}
TILE_LANE = np.dtype([("a", "<u4", 8), ("b", "<u4", 8), ("ea", "<i4"), ("eb", "<i4"), ("acc", "<f4", 4), ("expect", "<f4", 4)])


def hbm_data(nbytes, iters, device=0, seed=0x5EED):
    """(result, the copy buffer after the last of `iters` iterations as uint32 words)"""
    r, data = native().diag_hbm_data(device, nbytes, iters, seed)
    return json.loads(r), np.frombuffer(data, dtype="<u4")


def hbm_walk_data(nbytes, chunk_bytes, passes, device=0, seed=0x5EED):
    """(result with ``chunk_list``, the chunks' contents after `passes` passes, back to back, as
    uint64 words)"""
    r, data = native().diag_hbm_walk_data(device, nbytes, chunk_bytes, passes, seed)
    return json.loads(r), np.frombuffer(data, dtype="<u8")


def pcie_data(nbytes, device=0, seed=0x5EED):
    """(result, the host buffer after the round trip as uint64 words)"""
    r, data = native().diag_pcie_data(device, nbytes, seed)
    return json.loads(r), np.frombuffer(data, dtype="<u8")


def gemm_soak_data(m, n, k, device=0, seed=0x5EED):
    """(result, A m x k and Bt n x k as bf16 bit patterns, rref m and cref n as int64, C m x n fp32)
    of one launch"""
    r, a, bt, rref, cref, c = native().diag_gemm_soak_data(device, m, n, k, seed)
    return (json.loads(r), np.frombuffer(a, dtype="<u2").reshape(m, k), np.frombuffer(bt, dtype="<u2").reshape(n, k),
            np.frombuffer(rref, dtype="<i8"), np.frombuffer(cref, dtype="<i8"), np.frombuffer(c, dtype="<f4").reshape(m, n))


def mfma_tile(path, tile, scaled=False, device=0, seed=0x5EED):
    """What each of the 64 lanes holds for tile `tile` of the "bf16", "fp8" or "fp4" check: a
    record array of TILE_LANE (fragment dwords a and b, scale exponents ea and eb, the matrix
    core's acc and the check's expect)."""
    return np.frombuffer(native().diag_mfma_tile(device, TILE_PATHS[path], int(scaled), seed, tile), dtype=TILE_LANE)


CLASSIC_TILE_LANE = np.dtype([("a", "<u4", 4), ("b", "<u4", 4), ("acc", "<f8", 4), ("expect", "<f8", 4)])


def mfma_classic_tile(path, tile, device=0, seed=0x5EED):
    """What each of the 64 lanes holds for check tile `tile` of the "fp16", "int8", "fp32" or "fp64"
    path: a record array of CLASSIC_TILE_LANE (fragment dwords a and b, the matrix core's acc and
    the check's expect, both as doubles)."""
    return np.frombuffer(native().diag_mfma_classic_tile(device, _classic_path(path), seed, tile), dtype=CLASSIC_TILE_LANE)


def lds_data(wg, pass_, grid, device=0, seed=0x5EED):
    """The LDS_WORDS words that workgroup `wg` of a march of `grid` workgroups holds after pass
    `pass_` (0: the pattern, 1: its inverse), as uint32."""
    return np.frombuffer(native().diag_lds_data(device, seed, wg, pass_, grid), dtype="<u4")


def cache_data(passes, device=0, rounds=1, region_bytes=L2_REGION_BYTES, l2_sweeps=16, ic_bytes=2 << 20, ic_sweeps=2, seed=0x5EED):
    """(result, the L2 buffer as uint32 [cus, region words] as the march left it, its last round ended
    after `passes` (1 or 2) passes, the Infinity-Cache buffer as the last check saw it as uint32)"""
    r, l2, ic = native().diag_cache_data(device, rounds, region_bytes, passes, l2_sweeps, ic_bytes, ic_sweeps, seed)
    r = json.loads(r)
    return r, np.frombuffer(l2, dtype="<u4").reshape(r["cus"], region_bytes // 4), np.frombuffer(ic, dtype="<u4")


VALU_WAVE = np.dtype([("cu_key", "<i4"), ("simd", "<i4"), ("rate_cu_key", "<i4", 5), ("digests", "<u4", (7, 64)), ("raw", "<u4", (64, VALU_ROUND_WORDS, 64))])


def _valu_wave(data, rounds):
    w = np.frombuffer(data, dtype=VALU_WAVE)[0]
    return {"cu_key": int(w["cu_key"]), "simd": int(w["simd"]), "rate_cu_key": [int(k) for k in w["rate_cu_key"]], "digests": w["digests"], "raw": w["raw"][:rounds]}


def valu_data(wave, check_plants=(), rate_plants=(), delays=(), device=0, waves_per_simd=1, rounds=2, rate_iters=16, seed=0x5EED):
    """(result, check wave `wave` of that run) with the plants of valu_planted and the delays of valu_delayed applied.
    The wave: ``cu_key`` and ``simd`` where it ran in the check launch, ``rate_cu_key`` the CU it ran on in each rate
    class's timed launch (a wave is placed anew in every launch, and in every run), ``digests`` [class, lane] as it
    wrote them, ``raw`` [round, result word of the round, lane] as it folded them, all uint32."""
    check = [(p[0], _valu_code(VALU_CLASSES, p[1])) + tuple(p[2:]) for p in check_plants]
    rate = [(p[0], _valu_code(VALU_RATE_CLASSES, p[1])) + tuple(p[2:]) for p in rate_plants]
    slow = [(d[0], _valu_code(VALU_RATE_CLASSES, d[1]), d[2]) for d in delays]
    r, data = native().diag_valu_data(device, waves_per_simd, rounds, rate_iters, seed, wave, check, rate, slow)
    return json.loads(r), _valu_wave(data, rounds)


def valu_expected(rounds, seed=0x5EED):
    """What the host referee expects of every wave, shaped as valu_data's wave (``cu_key``, ``simd`` and ``rate_cu_key`` -1; the
    trans words are double-precision libm rounded to fp32, which no digest is compared with).  Needs no GPU."""
    return _valu_wave(native().diag_valu_expected(seed, rounds), rounds)


XLANE_WAVE = np.dtype([("cu_key", "<i4"), ("simd", "<i4"), ("rate_cu_key", "<i4", 4), ("digests", "<u4", (8, 64)), ("raw", "<u4", (64, XLANE_ROUND_WORDS, 64))])


def _xlane_wave(data, rounds):
    w = np.frombuffer(data, dtype=XLANE_WAVE)[0]
    return {"cu_key": int(w["cu_key"]), "simd": int(w["simd"]), "rate_cu_key": [int(k) for k in w["rate_cu_key"]], "digests": w["digests"], "raw": w["raw"][:rounds]}


def xlane_data(wave, check_plants=(), rate_plants=(), delays=(), device=0, waves_per_simd=1, rounds=2, rate_iters=16, seed=0x5EED):
    """(result, check wave `wave` of that run) with the plants of xlane_planted and the delays of xlane_delayed applied.
    The wave: ``cu_key`` and ``simd`` where it ran in the check launch, ``rate_cu_key`` the CU it ran on in each rate
    class's timed launch, ``digests`` [class, lane] as it wrote them, ``raw`` [round, result word of the round, lane] as
    it folded them, all uint32."""
    check = [(p[0], _valu_code(XLANE_CLASSES, p[1])) + tuple(p[2:]) for p in check_plants]
    rate = [(p[0], _valu_code(XLANE_RATE_CLASSES, p[1])) + tuple(p[2:]) for p in rate_plants]
    slow = [(d[0], _valu_code(XLANE_RATE_CLASSES, d[1]), d[2]) for d in delays]
    r, data = native().diag_xlane_data(device, waves_per_simd, rounds, rate_iters, seed, wave, check, rate, slow)
    return json.loads(r), _xlane_wave(data, rounds)


def xlane_expected(rounds, seed=0x5EED):
    """What the host referee expects of every wave, shaped as xlane_data's wave (``cu_key``, ``simd`` and ``rate_cu_key``
    -1).  Needs no GPU."""
    return _xlane_wave(native().diag_xlane_expected(seed, rounds), rounds)


ATOMIC_LAYOUT = np.dtype([("grid", "<i4"), ("rate_grid", "<i4"), ("rounds", "<i4"), ("waves", "<i4"), ("pairs", "<u4"), ("rows", "<u4", (2, 8)),
                          ("order_cap", "<u4", 3), ("table_off", "<u8", (2, 8)), ("data_off", "<u8", 8), ("data_words", "<u8", 8),
                          ("total_words", "<u8")])  # bgc_atomic_layout


def atomic_layout(grid, rounds, rate_grid=8):
    """Where everything of a check launch of `grid` workgroups lies (bgc_atomic_layout), as a numpy record.  Needs no GPU."""
    return np.frombuffer(native().diag_atomic_layout(grid, rate_grid, rounds), dtype=ATOMIC_LAYOUT)[0]


def _atomic_block(layout, data):
    """The sections of a data block: ``own`` and ``shared`` {class: [word, row, lane]; int64 and f64 [row, lane] uint64}, ``ballots``
    [own / shared / lds, pair] uint64, ``order`` {own, shared, lds: [row, lane, slot]}, ``cu_keys`` [workgroup], ``rate_cu_keys``
    [rate class, workgroup], and ``words``, the whole block."""
    words = np.frombuffer(data, dtype="<u4")
    assert words.size == int(layout["total_words"])

    def section(s):
        return words[int(layout["data_off"][s]):int(layout["data_off"][s]) + int(layout["data_words"][s])]

    out = {"words": words, "layout": layout}
    for pl, name in enumerate(ATOMIC_PLACEMENTS):
        table, classes = section(pl), {}
        for c, cls in enumerate(ATOMIC_CLASSES):
            rows, first = int(layout["rows"][pl][c]), int(layout["table_off"][pl][c])
            part = table[first:first + rows * 64 * ATOMIC_CLASS_WORDS[c]]
            classes[cls] = part.view("<u8").reshape(rows, 64) if cls in ("int64", "f64") else part.reshape(ATOMIC_CLASS_WORDS[c], rows, 64)
        out[name] = classes
    out["ballots"] = section(2).view("<u8").reshape(3, int(layout["pairs"]))
    out["order"] = {name: section(3 + k).reshape(-1, 64, int(layout["order_cap"][k])) for k, name in enumerate(("own", "shared", "lds"))}
    out["cu_keys"] = section(6).view("<i4")
    out["rate_cu_keys"] = section(7).view("<i4").reshape(4, int(layout["rate_grid"]))
    return out


def atomic_data(plants=(), rate_plants=(), delays=(), device=0, wgs_per_cu=1, rounds=2, rate_iters=15, seed=0x5EED):
    """(result, data of that run) with the plants of atomic_planted and the delays of atomic_delayed applied: the final tables, the
    winners' ballots, the order arrays and the CU key that every workgroup recorded, in the check launch and in each timed rate
    launch (see _atomic_block)."""
    r, data = native().diag_atomic_data(device, wgs_per_cu, rounds, rate_iters, seed, _atomic_plants(plants), _atomic_rate_plants(rate_plants),
                                        _atomic_rate_plants(delays))
    r = json.loads(r)
    return r, _atomic_block(atomic_layout(r["cus"] * wgs_per_cu, rounds, (2 * r["cus"] + 7) // 8 * 8), data)


def atomic_expected(grid, rounds, plants=(), seed=0x5EED):
    """The host referee's tables for a launch of `grid` workgroups with `plants` applied, shaped as atomic_data's (the CU keys
    -1).  Every cas goes to the contender with the lowest pair and every ticket is drawn in the order of the pairs: one admissible
    outcome of what the hardware's order decides.  Needs no GPU."""
    return _atomic_block(atomic_layout(grid, rounds), native().diag_atomic_expected(seed, grid, rounds, _atomic_plants(plants)))


def atomic_rate_expected(rate_grid, rate_iters, cls, seed=0x5EED):
    """The end values of rate class `cls` for `rate_grid` workgroups: [group, row, lane] uint32 (f32: float bits; pk_bf16: packed),
    or the groups' heads of "rtn".  Needs no GPU."""
    code = _valu_code(ATOMIC_RATE_CLASSES, cls)
    out = np.frombuffer(native().diag_atomic_rate_expected(seed, rate_grid, rate_iters, code), dtype="<u4")
    return out if code == 3 else out.reshape(-1, 64, 64)


REGFILE_LAYOUT = np.dtype([("regs", "<i4"), ("lanes", "<i4"), ("temps", "<i4"), ("ring_regs", "<i4"), ("plant_slots", "<i4"),
                           ("marched", "u1", (2, 512)), ("temp_regs", "<i4", (2, 8)), ("ring", "<i4", 512), ("plant_regs", "<i4", 8),
                           ("plant_phase_ok", "u1", (8, 5))])  # bgc_regfile_layout
REGFILE_PLACE = np.dtype([("cu_key", "<i4"), ("simd", "<i4")])  # bgc_regfile_place


def regfile_layout():
    """The two march layouts, the rotate's ring and the plant registers (bgc_regfile_layout), as a numpy record: ``marched``
    [layout, register], ``temp_regs`` [layout], ``ring`` (its first ``ring_regs`` entries: ring index -> register),
    ``plant_regs`` [slot] and ``plant_phase_ok`` [slot, phase].  Needs no GPU."""
    return np.frombuffer(native().diag_regfile_layout(), dtype=REGFILE_LAYOUT)[0]


def regfile_data(wave, phase, plants=(), delays=(), device=0, wgs_per_cu=1, sweeps=3, seed=0x5EED):
    """(result, words, march_places, rotate_places) of a run with the plants of regfile_planted and the delays of regfile_delayed:
    wave `wave`'s whole file as phase `phase` had it, [register, lane] uint32 (after the fill and the plants of a march phase,
    or after the timed rotate's sweeps; the phase's own eight registers are 0), and the (``cu_key``, ``simd``) every wave
    recorded in the march launch and in the timed rotate launch of this very run."""
    r, words, march, rotate = native().diag_regfile_data(device, wgs_per_cu, sweeps, seed, wave, phase, [tuple(p) for p in plants],
                                                         [tuple(d) for d in delays])
    return (json.loads(r), np.frombuffer(words, dtype="<u4").reshape(REGFILE_REGS, 64), np.frombuffer(march, dtype=REGFILE_PLACE),
            np.frombuffer(rotate, dtype=REGFILE_PLACE))


def regfile_expected(wave, phase, sweeps=3, plants=(), seed=0x5EED):
    """What regfile_data returns as `words` for that wave, phase, sweep count and plants, from the host reference
    (regfile_ref.h): after `sweeps` sweeps ring index i holds what the fill and the plants put at index (i + sweeps) mod
    ring_regs.  Needs no GPU."""
    return np.frombuffer(native().diag_regfile_expected(seed, wave, phase, sweeps, [tuple(p) for p in plants]), dtype="<u4").reshape(REGFILE_REGS, 64)


def _bf16_bytes(x):
    """bf16 bits of a float array / tensor (round to nearest even), row-major."""
    try:
        import torch
        if isinstance(x, torch.Tensor):
            return x.detach().to("cpu", torch.bfloat16).contiguous().view(torch.int16).numpy().tobytes()
    except ImportError:
        pass
    f = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((f + 0x7FFF + ((f >> 16) & 1)) >> 16).astype(np.uint16).tobytes()


def gemm(a, b, device=0):
    """C = A @ B on the one-wave-per-tile MFMA kernel (dense_gemm).  A is MxK, B is KxN; M and N
    must be multiples of 16 (up to 4096) and K of 32 (up to 8192).  Returns an fp32 numpy array
    MxN."""
    m, k = a.shape
    k2, n = b.shape
    if k != k2:
        raise ValueError(f"inner dimensions differ: A is {m}x{k}, B is {k2}x{n}")
    c = native().diag_gemm(device, m, n, k, _bf16_bytes(a), _bf16_bytes(b))
    return np.frombuffer(c, dtype=np.float32).reshape(m, n)


def gemm_dtype(a, b, path, device=0):
    """C = A @ B on classic path `path` ("fp16", "int8", "fp32", "fp64"), one wave per 16x16 tile
    (dense_gemm).  A is MxK, B is KxN, converted to the path's element type; M and N must be
    multiples of 16 (up to 4096) and K of the path's K (up to 8192).  Returns a float64 numpy array
    MxN, which holds every path's results exactly."""
    m, k = a.shape
    k2, n = b.shape
    if k != k2:
        raise ValueError(f"inner dimensions differ: A is {m}x{k}, B is {k2}x{n}")
    dt = CLASSIC_DTYPES[path]
    c = native().diag_gemm_dtype(device, CLASSIC_PATHS[path], m, n, k, np.ascontiguousarray(a, dtype=dt).tobytes(),
                                 np.ascontiguousarray(b, dtype=dt).tobytes())
    return np.frombuffer(c, dtype=np.float64).reshape(m, n)


def gemm_tiled(a, bt, device=0):
    """C = A @ Bt^T on the soak's kernels.  A is MxK, Bt is NxK; M and N must be
    multiples of 128 and K of 64 (the ping-pong kernel runs when M, N are multiples of
    256 and K of 128).  Returns an fp32 numpy array MxN."""
    m, k = a.shape
    n, k2 = bt.shape
    if k != k2:
        raise ValueError(f"inner dimensions differ: A is {m}x{k}, Bt is {n}x{k2}")
    c = native().diag_gemm_tiled(device, m, n, k, _bf16_bytes(a), _bf16_bytes(bt))
    return np.frombuffer(c, dtype=np.float32).reshape(m, n)


def mx_gemm(a, a_scales, bt, bt_scales, fmt="fp8", device=0):
    """C = sum_k a[m,k] 2^(sa[m,k/32]-127) * bt[n,k] 2^(sbt[n,k/32]-127) on the MX matrix
    cores (v_mfma_scale_f32_16x16x128_f8f6f4).  fp8: `a` M x K and `bt` N x K uint8 e4m3
    codes; fp4: M x K/2 and N x K/2 bytes of packed e2m1 codes (element 2i in the low
    nibble).  Scales: uint8 E8M0, M x K/32 and N x K/32.  M, N multiples of 16, K of 128.
    Returns an fp32 numpy array M x N."""
    code = {"fp8": 0, "fp4": 4}[fmt]
    a, bt = np.ascontiguousarray(a, dtype=np.uint8), np.ascontiguousarray(bt, dtype=np.uint8)
    sa, sb = np.ascontiguousarray(a_scales, dtype=np.uint8), np.ascontiguousarray(bt_scales, dtype=np.uint8)
    m, n = a.shape[0], bt.shape[0]
    k = sa.shape[1] * 32
    c = native().diag_mx_gemm(device, code, m, n, k, a.tobytes(), sa.tobytes(), bt.tobytes(), sb.tobytes())
    return np.frombuffer(c, dtype=np.float32).reshape(m, n)
