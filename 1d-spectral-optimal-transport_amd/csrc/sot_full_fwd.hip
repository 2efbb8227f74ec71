// sot_full_fwd.hip -- full-row forward kernels for compile-time row lengths, and which row lengths the full-row kernels take;
// the kernel and launch templates are in sot_full_fwd.hpp.
#include "sot_full_fwd.hpp"

namespace sot {

// Preconditions: those of dispatch_forward_full, plus p == 1, no quantile cutoff, SOT_FLAG_SAME_GRID.
hipError_t dispatch_area_full(const FwdArgs& a, hipStream_t s)
{
    switch (a.n) {
        case 8192: return dispatch_area_full_g<1024, 8, 1>(a, s);
        case 129:   // two rows per wave: 65536 rows 25.3 -> 20.6 us, 4096 rows 7.9 -> 7.7 us
            return dispatch_area_half<5, 8, 129>(a, s);
        case 2049: return dispatch_area_full_g<256, 9, 1, 2049>(a, s);
        case 257:   // (two rows per wave: 65536 rows 33.0 -> 32.0 us, 16384 rows 10.2 -> 10.8 us: this kernel is at the HBM limit for 257-bin rows already)
            return dispatch_area_full_g<64, 5, 4, 257>(a, s);
        case 513: return dispatch_area_full_g<64, 9, 4, 513>(a, s);
        case 1025:   // one wave per row (17 elements per thread, no workgroup barrier): 1024 / 4096 rows as before (7.4 / 10.7 us), 8192 rows 18.7 -> 16.9 us,
                     // 16384 rows 31.3 -> 29.2 us against <128, 9, 2> (interleaved A/B)
            return dispatch_area_full_g<64, 17, 4, 1025>(a, s);
        default: return dispatch_area_full_pow2<float>(a, s);   // 512 ... 4096 bins: the table shared with the 16-bit rows (sot_full_fwd.hpp)
    }
}

hipError_t dispatch_forward_full_rowpos(int pm, const FwdArgs& a, hipStream_t s)
{
    switch (a.n) {
        case 2048: return dispatch_forward_full_rowpos_g<256>(pm, a, s);
        case 1024: return dispatch_forward_full_rowpos_g<128>(pm, a, s);
        case 512: return dispatch_forward_full_rowpos_g<64>(pm, a, s);
        default: return hipErrorInvalidConfiguration;
    }
}

// Run-time row lengths (NX = -1): any n == m <= 8192 on shared positions runs the compile-time GEOMETRY of the next capacity
// (256 / 512 / 1024 / 2048 / 4096 / 8192 points; the backward up to 4096).  Replaces the generic kernels for such rows:
// 8192 x 2000 forward 70 -> ~50 us, training form 192 -> ~90 us.
int full_rt_capacity(int n)
{
    if (n <= 128) return 0;    // tiny rows: the generic (64, 8) kernel wastes less
    for (int cap = 256; cap <= 8192; cap <<= 1) {
        // 1536 = 192 x 8, 3072 = 384 x 8: rows just above a power of two do not pay for twice their length
        if (cap >= 2048 && cap <= 4096 && n <= cap - cap / 4) return cap - cap / 4;
        if (n <= cap) return cap;
    }
    return 0;
}

// Row lengths with a compile-time kernel: 512 / 1024 / 2048 / 4096 / 8192 bins (16-B aligned rows required) and the
// one-sided spectra of n_fft 256 ... 4096: 129 / 257 / 513 / 1025 / 2049 bins (the paper uses 257 and 1025; any alignment).
bool forward_full_supports(int n, bool aligned16)
{
    return ((n == 512 || n == 1024 || n == 2048 || n == 4096 || n == 8192) && aligned16) || n == 129 || n == 257 || n == 513 ||
           n == 1025 || n == 2049;
}

// The caller (run_forward) guarantees: shared positions, n == m with forward_full_supports(n, ...), p in {1, 2}, not
// pre-normalised.  LDS size, block size and grid are this kernel's own (shared-position layout).
hipError_t dispatch_forward_full(int pm, const FwdArgs& a, hipStream_t s)
{
    switch (a.n) {
        case 8192: return dispatch_forward_full_g<1024, 8, 1>(pm, a, s);
        case 129:   // large batches: two rows per wave (sot_forward_half_kernel).  Paper mode, interleaved A/B: 8192 rows 7.5 -> 6.9 us, 16384 rows 11.7 -> 10.4,
                    // 32768 rows 19.8 -> 16.0, 65536 rows 35.0 -> 28.0 us
            if (a.B >= 8192) return dispatch_forward_half<5, 8, 129>(pm, a, s);
            return dispatch_forward_full_g<64, 3, 4, 129>(pm, a, s);
        case 2049: return dispatch_forward_full_g<256, 9, 1, 2049>(pm, a, s);
        case 257:   // the same from ~40 000 rows: 16384 rows 15.5 -> 16.8 us, 32768 rows 25.6 -> 26.4, 49152 rows 40.4 -> 37.4, 65536 rows 53.0 -> 47.8 us
                    // (each row region carries its own copy of the positions -- the walk addresses a level's position at a constant offset -- so
                    // LDS holds 32 rows = 16 waves per CU: fewer, longer-running waves than the one-wave kernel, which only pays once the launch is long)
            if (a.B >= 40960) return dispatch_forward_half<9, 8, 257>(pm, a, s);
            return dispatch_forward_full_g<64, 5, 4, 257>(pm, a, s);
        case 513: return dispatch_forward_full_g<64, 9, 4, 513>(pm, a, s);
        case 1025:
            // Large batches: ONE wave per row (17 elements per thread, four rows per workgroup, no workgroup barrier anywhere in the row).
            // Interleaved A/B against two waves per row, paper mode: 1024 rows 7.5 -> 8.4 us, 4096 rows 15.5 -> 15.5, 6144 rows 20.3 ->
            // 19.3, 8192 rows 25.6 -> 23.3, 12288 rows 35.3 -> 31.6, 16384 rows 45.1 -> 42.2 us.  (Its thread-local sums group the row
            // differently: row losses agree with the two-wave kernels' to ~1e-7, not bit for bit.  The training kernel in this
            // geometry needs 17-element gradient arrays in registers and is slower: 85 -> 107 us at 16384 rows.)
            if (a.B >= kFwd1025OneWaveRows) return dispatch_forward_full_g<64, 17, 4, 1025>(pm, a, s);
            return dispatch_forward_full_g<128, 9, 2, 1025>(pm, a, s);  // 256 threads per row: 64.6 instead of 54.4 us at 16384 rows (round 1)
        default: return dispatch_forward_full_pow2<float>(pm, a, s);   // 512 ... 4096 bins: the table shared with the 16-bit rows (sot_full_fwd.hpp)
    }
}

// Same preconditions as dispatch_forward_full, without 8192-bin rows (8192 + 8192 bins with gradient arrays exceed the LDS);
// for 512 / 2048 bins the gradient buffers must be 16-B aligned as well.
bool backward_full_supports(int n, bool aligned16) { return n != 8192 && forward_full_supports(n, aligned16); }

}  // namespace sot
