/* hipbe.h -- the E-step backend of the host driver bound to libpsmc_hip.so (include/psmc_hip.h): what `psmc` and the main
 * run of `psmc_boot --main` hand to psmc_run().  Compiled into the executables, not into libpsmc_host.so (which stays
 * free of GPU code: the CPU tests link it against the oracle instead). */
#ifndef PSMC_HIPBE_H
#define PSMC_HIPBE_H
#include "psmc_host.h"
#include "psmc_hip.h"

/* One context on `device` (devices == NULL or without a comma) or the segments of every E-step sharded over the listed
 * devices (psmc_hip_group_*).  use_factored: hand psmc_run the factored E-step (fast mode + O(N) objective).
 * Returns 0 or a PSMC_HIP_E* code; be->destroy releases everything. */
int psmc_hipbe_create(psmc_estep_backend *be, int n_states, int mode, int use_factored, const char *devices, int device);
/* psmc_hip_set_option / psmc_hip_group_set_option on the backend's context or group */
int psmc_hipbe_set_option(psmc_estep_backend *be, const char *key, double value);
/* The note `psmc` prints on stderr about its full-count E-steps on the wide fast path (PSMC_HIP_WIDE_COUNTS=1): held back until the
 * first E-step has run, so that it can say what that E-step kept -- ", X at every 8th bin" is appended when it kept checkpoints
 * ("wide_ckpt" + "wide_counts_ckpt" through PSMC_HIP_OPTIONS).  `line` has no newline; the backend copies it. */
void psmc_hipbe_note_counts(psmc_estep_backend *be, const char *line);
/* the single context behind the backend (NULL for a sharded one): psmc_hip_set_cu_range, psmc_hip_reserve_tables */
psmc_hip_ctx *psmc_hipbe_ctx(psmc_estep_backend *be);
#endif
