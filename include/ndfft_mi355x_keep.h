/*
 * ndfft_mi355x_keep.h -- the kept share of a streamed input (ABI minor 7): one diagnostic and two per-thread settings.  C99; included by
 * ndfft_mi355x_ext.h, whose own list of entry points stays what it was at minor 6.
 *
 * A dense C2C row call that streams its input (ndfft_last_input_policy() == 1) may still load keep / 64 of it -- a fixed, evenly spread set of
 * 64 KiB blocks -- with the default cache policy, so that a recurring input larger than the Infinity Cache finds that part resident the next
 * time round.  Speed only: the same bits either way.
 */
#ifndef NDFFT_MI355X_KEEP_H
#define NDFFT_MI355X_KEEP_H

#include "ndfft_mi355x.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Diagnostic beside ndfft_last_input_policy(): the kept share of the last device exec on this thread, 0 .. 64.  0: nothing kept, or no such call. */
int ndfft_last_input_keep(void);
/* The Infinity-Cache budget, in MiB, that the kept shares of the members of a rotation add up to, for this host thread: 0 switches the kept share off (every
 * streamed input streams whole), a negative value restores the library's default.  For A/B runs; NDFFT_ERR_INVALID_ARG beyond 2^20. */
int ndfft_set_keep_budget(int mib);
/* Test and sweep hook, per host thread: every dense C2C row call that streams its input -- by the model, the hint or NDFFT_STREAM_LOADS -- keeps keep64 (0 .. 64)
 * of every 64 blocks, whatever the model would grant; a negative value gives the decision back to the model.  NDFFT_ERR_INVALID_ARG beyond 64. */
int ndfft_force_input_keep(int keep64);

#ifdef __cplusplus
}
#endif
#endif /* NDFFT_MI355X_KEEP_H */
