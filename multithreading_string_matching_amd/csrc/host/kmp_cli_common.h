/*
 * kmp_cli_common.h -- what bin/serial, bin/openmp_data (kmp_cli.c) and bin/openmp_task (kmp_cli_task.c) have in common: the clock,
 * the exit on a GPU error, the protocol argument, the environment variables both read, the pattern upload and the count reduce over
 * the shards.  Static functions: each program includes this header once, after kmpgpu.h and kmphost.h.
 */
#ifndef KMP_CLI_COMMON_H
#define KMP_CLI_COMMON_H

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "kmpgpu.h"
#include "kmphost.h"

static inline double now_s(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec;
}

static inline void die_gpu(const char *what)
{
    fprintf(stderr, "%s: %s\n", what, kmpgpu_last_error());
    exit(2);
}

static inline int parse_proto(const char *s, int *proto)
{
    if (strcmp(s, "udp") == 0) { *proto = KMP_PROTO_UDP; return 1; }       /* serial.c:38-41 */
    if (strcmp(s, "tcp") == 0) { *proto = KMP_PROTO_TCP; return 1; }
    return 0;
}

/* NAME=1, exactly (KMPGPU_WHOLE_PAYLOAD, KMPGPU_NOCASE) */
static inline int env_flag(const char *name)
{
    const char *e = getenv(name);
    return e && e[0] == '1' && e[1] == 0;
}

/* NAME=<path>; NULL when the variable is unset or empty */
static inline const char *env_path(const char *name)
{
    const char *e = getenv(name);
    return e && e[0] ? e : NULL;
}

/* the two older switches, each with the looser test it always had */
static inline int env_device_extract(void)
{
    const char *e = getenv("KMPGPU_DEVICE_EXTRACT");
    return e && e[0] == '1';
}

static inline int env_stats(void)
{
    const char *e = getenv("KMPGPU_STATS");
    return e && e[0] && e[0] != '0';
}

/* The patterns of a context, as the environment wants them matched; every context of a run passes through here.
 * whole_payload (KMPGPU_WHOLE_PAYLOAD=1): payloads are matched to their ends, not to their first 0x00 (KMPGPU_OPT_WHOLE_PAYLOAD).
 * nocase (KMPGPU_NOCASE=1): every pattern is matched case-insensitively (ASCII letters, KMPGPU_PAT_NOCASE); the report prints the
 * tokens as written. */
static inline int set_patterns_env(kmpgpu_ctx *c, const uint8_t *const *pp, const uint32_t *len, uint32_t n, int whole_payload, int nocase)
{
    if (whole_payload && kmpgpu_set_option(c, KMPGPU_OPT_WHOLE_PAYLOAD, 1)) return KMPGPU_EINVAL;
    if (!nocase || n == 0) return kmpgpu_set_patterns(c, pp, len, n);
    uint32_t *fl = (uint32_t *)malloc(n * sizeof *fl);
    if (!fl) return KMPGPU_ENOMEM;
    for (uint32_t i = 0; i < n; i++) fl[i] = KMPGPU_PAT_NOCASE;
    const int rc = kmpgpu_set_patterns_flags(c, pp, len, fl, n);
    free(fl);
    return rc;
}

/* KMPGPU_STATS=1: which rule bounded the text of a payload */
static inline void print_text_rule(int whole_payload)
{
    fprintf(stderr, "[kmpgpu] text rule: %s\n", whole_payload ? "whole payloads (KMPGPU_WHOLE_PAYLOAD=1)" : "up to a payload's first NUL (the reference's strlen)");
}

/* The count reduce over the shards (mpi_dumping.c:202), in two steps because bin/serial and bin/openmp_data bring the communicator up
 * before they start the clock of their scan passes.
 *
 * reduce_comm: one shard per device -> a communicator for an RCCL all-reduce over xGMI of the shards' device counters
 * (kmpgpu_comm_*); shards that share a device (more shards than GPUs) -> NULL, the host sums.  KMPGPU_RCCL=0 forces the host sum,
 * =1 asks for the communicator even with a single shard.  No communicator is no reason to stop: NULL then, too.  The caller destroys
 * what it gets. */
static inline kmpgpu_comm *reduce_comm(kmpgpu_ctx **ctxs, int shards, int ndev)
{
    const char *rccl_env = getenv("KMPGPU_RCCL");
    kmpgpu_comm *comm = NULL;
    if (!(shards <= ndev && (shards > 1 || (rccl_env && rccl_env[0] == '1')) && !(rccl_env && rccl_env[0] == '0'))) return NULL;
    if (kmpgpu_comm_init(&comm, ctxs, shards)) {
        fprintf(stderr, "[kmpgpu] kmpgpu_comm_init: %s -- summing the shards' counts on the host\n", kmpgpu_last_error());
        return NULL;
    }
    return comm;
}

/* reduce_counts: every shard's own counts go to own[r * n_patterns ...] first -- the offsets file needs them again, and they are what
 * the host sums without a communicator or should the all-reduce fail (n_patterns x 8 bytes per shard).  With a communicator the device
 * counters are then summed in place and downloaded ONCE, from shard 0 (MPI_Reduce root 0).  counts[] gets the totals; returns whether
 * RCCL made them. */
static inline int reduce_counts(kmpgpu_ctx **ctxs, int shards, uint32_t n_patterns, uint64_t *own, uint64_t *counts, kmpgpu_comm *comm)
{
    for (int r = 0; r < shards; r++)
        if (kmpgpu_counts_read(ctxs[r], own + (size_t)r * n_patterns)) die_gpu("kmpgpu_counts_read");
    if (comm) {
        int bad = kmpgpu_comm_allreduce_counts(comm) != 0;
        if (!bad) bad = kmpgpu_counts_read(ctxs[0], counts) != 0;
        for (int r = 1; r < shards && !bad; r++) bad = kmpgpu_sync(ctxs[r]) != 0;
        if (!bad) return 1;
        fprintf(stderr, "[kmpgpu] RCCL all-reduce of the counts: %s -- summing the shards' counts on the host\n", kmpgpu_last_error());
    }
    for (uint32_t i = 0; i < n_patterns; i++) {
        counts[i] = 0;
        for (int r = 0; r < shards; r++) counts[i] += own[(size_t)r * n_patterns + i];        /* mpi_dumping.c:202 MPI_SUM */
    }
    return 0;
}

#endif
