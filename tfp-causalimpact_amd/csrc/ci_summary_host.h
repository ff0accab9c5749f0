// ci_summary_host.h -- what ci_summary.hip defines for the other host unit that summarises through
// a session's scratch (ci_forecast.hip).  Internal: not installed.
#pragma once
#include "ci_session.h"

// num_ranks in [1, SUMM_MAX_RANKS], every rank in [0, N).
int check_ranks(int32_t num_ranks, const int32_t* ranks, int N);

// Order statistics of the rows of two [rows, N] matrices in one launch (M1 may be NULL: one
// matrix); out[(row / T) * R + r][row % T].  The select kernels are instantiated in ci_summary.hip.
hipError_t launch_select(hipStream_t stream, int N, int T, int rows, int R, const int* d_ranks,
                         const double* M0, const double* M1, double* out0, double* out1);

// The scratch of a summary of B series of N draws over T steps: allocated on first use and kept.
int summ_scratch_alloc(SummScratch& w, int B, int T, int N);

// The group table of the pool entry points (CSR over the positions of the session's B series).
int check_groups(int B, int32_t G, const int32_t* offsets, const int32_t* members, const double* weights);
