/* Counter-based sampler noise; included by lb_hip.h, which describes it next to the step kernels.  The launcher takes a stream
 * and can be recorded into a program (hip/lib.py: NOISE_SIGNATURES). */
#ifndef LB_HIP_NOISE_H
#define LB_HIP_NOISE_H
#ifdef __cplusplus
extern "C" {
#endif
/* rows_dev: uint32[n][8] = {key0, key1, ctr1, ctr2, ctr3, 0, 0, 0} (32-byte rows); out: fp16 [n][per_sample].
 * Element e of row j is word e % 4 of Philox4x32-10(ctr = {e / 4, ctr1, ctr2, ctr3}, key = {key0, key1}) (Random123:
 * multipliers 0xD2511F53 / 0xCD9E8D57, Weyl constants 0x9E3779B9 / 0xBB67AE85, ten rounds), turned into normals in pairs -
 * words (w0, w1) give elements 0 and 1, (w2, w3) elements 2 and 3:
 *   u1 = ((wa >> 8) + 0.5) 2^-24;  t = ((wb >> 8) + 0.5) 2^-23;  r = sqrt(-2 ln u1);  z_even = r cospi(t);  z_odd = r sinpi(t)
 * evaluated in float64 and rounded once to fp16 (nearest even); |z| <= 5.89.  A value depends on its row's five words and its
 * index e alone: not on n, on the row's position j, on `out`, on the stream or on any launch before it.
 * raw = 1 (tests, tools): out is uint32 [n][per_sample] holding the Philox words themselves, same indexing.
 * Refused before anything is launched or recorded: n <= 0; per_sample <= 0 or not a multiple of 8; null or 16-byte-misaligned
 * rows_dev / out; per_sample / 4 >= 2^32.  Reads nothing but rows_dev[0 : 8 n], writes nothing outside out[0 : n per_sample].
 * rows_dev is read when the kernel RUNS: a recorded op reads it at every replay, like every operand a launcher records, so the
 * rows must stay allocated for as long as the program lives - and rewriting them between replays is how a program draws other
 * noise. */
int lb_counter_noise_f16(const void* rows_dev, void* out, long per_sample, int n, int raw, void* stream);
#ifdef __cplusplus
}
#endif
#endif
