// Goldilocks NTT passes, v2: radix-16 butterflies held in registers (gfx950).
//
// Why: tools/microbench_valu.hip shows the NTT is bound by integer VALU issue, not by HBM or LDS
// (a 64-bit mod-mul is ~17-26 VALU ops at ~4.2 cycles each).  The reference's generator makes every
// root of unity of order <= 64 a power of two (w_64 = 2^39, w_16 = 2^156 = -2^60, w_4 = 2^48; 2^96 = -1),
// so a 16-point DFT needs no general multiplication: its 17 non-trivial twiddles are shifts + one fold.
// A thread keeps 16 points in registers for four layers; general twiddles (tables) appear only between
// radix-16 stages, and LDS is touched once per stage instead of once per layer.
//
// Pass structure and dispatch: ntt_passes.hpp and lde_passes.hpp (the LDE's strided passes, PA), shared with BabyBear.  What is
// Goldilocks' own: the register DFTs (Dft<GlF>, dft_gl.hpp) and the LDE's contiguous pass PB (12 bits, natural -> leaf order).
#include "kernels.hpp"
#include "gl_field.hpp"
#include "ntt_passes.hpp"
#include "dft_gl.hpp"
#include "lde_passes.hpp"

namespace gbk {

// ------------------------------------------------------------------ LDE pass B: 4096 contiguous points, 3 radix-16 stages
// grid = number of 4096-tiles of `lde` (in place).  natural -> bit-reversed.
// The inter-stage twiddles cost as much as the butterflies here (ablations in DESIGN.md: without their loads and products the pass
// runs 33 % faster, close to a plain copy): the first stage reads them from a copy of the table laid out [slot][tid] (coalesced),
// the second from a 256-entry table in LDS.
__global__ __launch_bounds__(THREADS) void k_gl_lde_pb16(u64* __restrict__ lde, const u64* __restrict__ tw4096) {
    __shared__ u64 sh[16 * 272];
    __shared__ u64 tw2[256];  // the stage-2 twiddles as the threads read them: tw2[s][d0] = w_256^(brev4(s) d0) - consecutive lanes,
                              // consecutive words (indexed by exponent, slots with brev4(s) = 4, 8, 12 were 2- and 4-way bank conflicts)
    u64* p = lde + ((size_t)blockIdx.x << 12);
    const u32 tid = threadIdx.x;
    tw2[tid] = tw4096[((brev4(tid >> 4) * (tid & 15)) & 255) * 16];
    u64 x[16];
    // stage 1: digit d2 (stride 256); this thread is (d1, d0) = tid
#pragma unroll
    for (u32 d = 0; d < 16; d++) x[d] = p[d * 256 + tid];
    u64 tw[16];
#pragma unroll
    for (u32 s = 1; s < 16; s++) tw[s] = tw4096[4096 + s * 256 + tid];  // w_4096^(k2 (16 d1 + d0)), k2 = brev4(s)
    dft16<false>(x);
#pragma unroll
    for (u32 s = 0; s < 16; s++) sh[s * 272 + tid] = s ? gl::mul_mont(x[s], tw[s]) : x[s];
    __syncthreads();
    // stage 2: digit d1; this thread is (k2 slot, d0)
    const u32 hi4 = tid >> 4, lo4 = tid & 15;
#pragma unroll
    for (u32 d = 0; d < 16; d++) x[d] = sh[hi4 * 272 + d * 16 + lo4];
    dft16<false>(x);
    __syncthreads();
#pragma unroll
    for (u32 s = 0; s < 16; s++)   // w_256^(k1 d0) from LDS; [k2 slot][d0][k1 slot], rows padded to 17
        sh[hi4 * 272 + lo4 * 17 + s] = s ? gl::mul_mont(x[s], tw2[s * 16 + lo4]) : x[s];
    __syncthreads();
    // stage 3: digit d0; this thread is (k2 slot, k1 slot)
#pragma unroll
    for (u32 d = 0; d < 16; d++) x[d] = sh[hi4 * 272 + d * 17 + lo4];
    dft16<false>(x);
    __syncthreads();
    // x[s] belongs at tile position tid * 16 + s: transpose through LDS for a coalesced store
#pragma unroll
    for (u32 s = 0; s < 16; s++) sh[tid * 17 + s] = x[s];
    __syncthreads();
#pragma unroll
    for (u32 it = 0; it < 16; it++) {
        const u32 q = it * 256 + tid;
        p[q] = sh[(q >> 4) * 17 + (q & 15)];
    }
}

// ------------------------------------------------------------------ launchers (called from lde_columns<GlF> / lde_pa_r16<GlF>)
// Every LDE kernel takes the MONTGOMERY-form copies of the tables (GlNttTables::*_m, GlCosetTables::*_m): all of their general
// multiplications have a table value as one factor (gl::mul_mont).

// 2^22 rows: the two-stage pass with 32 x 32 points (lde_passes.hpp), 512 threads - a site that only Goldilocks reaches
void lde_pa_rows22(const u64* coeffs, u64* lde, size_t ncols, const GlNttTables& t, const GlCosetTables& ct, hipStream_t stream) {
    const LdeTables<GlF> tt = lde_tables(t, ct);
    hipLaunchKernelGGL((k_lde_pa32<GlF, 2>), dim3((u32)(ncols << 8)), dim3(512), 0, stream, coeffs, lde, ct.rate_bits, tt.tw4096, tt.tw_hi,
                       tt.tw_lo, tt.pow_lo, tt.pow_hi);
}

void lde_pb_r16(u64* lde, size_t ntiles, const GlNttTables& t, hipStream_t stream) {
    hipLaunchKernelGGL(k_gl_lde_pb16, dim3((u32)ntiles), dim3(THREADS), 0, stream, lde, t.tw4096_fwd_m);
}

GB_INSTANTIATE_NTT(GlF)

}  // namespace gbk
