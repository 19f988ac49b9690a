/*
 * dgj2t.h — C ABI of the MI355X-native batched JSON -> Thrift-binary
 * transcoder (the conv/j2t hot path of cloudwego/dynamicgo).
 *
 * Boundary replaced (reference, Go -> machine code, no cgo):
 *   J2T_FSM(fsm *types.J2TStateMachine, buf *[]byte, src *string, flag uint64) uint64
 *     internal/native/dispatch_amd64.go:66-68
 *   -> uint64_t j2t_fsm_exec(J2TStateMachine*, GoSlice *buf, const GoString *src, uint64_t flag)
 *     native/thrift.h:202, native/thrift.c:765-1187
 * and the Go prelude/epilogue around it (BinaryConv.do conv/j2t/impl.go:38-91,
 * BinaryConv.Do conv/j2t/conv.go:53-77).
 *
 * The reference converts ONE message per call, reading Go descriptor structs
 * in place. This ABI converts a BATCH: a JSON arena with n+1 offsets, against a
 * descriptor flattened once (include/dgj2t_desc.h) and kept resident on the
 * device. Per message it returns the Thrift bytes and the reference's packed
 * status word, bit-identical: code bits 0-7 | pos bits 8-39 | value bits 40-63
 * (native/thrift.h:223-242, decoded by explainNativeError
 * conv/j2t/impl_amd64.go:261-298), 0 = success.
 *
 * Flags are the reference's j2t flag word (native/thrift.h:23-32,
 * conv/j2t/conv.go:98-127 toFlags). DG_F_VALIDATE_UTF8 is an opt-in extension
 * (bit 16) that the reference does not have; off by default. With it, the raw
 * JSON bytes of every string written as a Thrift STRING (string values and
 * STRING map keys; not binary fields, not field-name keys) must be valid UTF-8
 * as utf8_validate (native/utf8.c:101-212) defines it; otherwise the message
 * fails with ERR_INVAL (2), value = the first byte of the invalid sequence,
 * pos = its offset.
 *
 * All functions return 0 on success and a negative DG_E_* on API failure;
 * dg_last_error() describes the last failure of the calling thread.
 */
#ifndef DGJ2T_H
#define DGJ2T_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#include "dgj2t_defs.h"

typedef struct dg_ctx dg_ctx;
typedef struct dg_desc dg_desc;
typedef struct dg_agg dg_agg;

/* Per-thread description of the last failure. */
const char *dg_last_error(void);

/* "dgj2t-build:<source sha256/16> arch:gfx950": what this library was built
 * from (dynamicgo_amd/build.py); no reference counterpart. */
const char *dg_build_info(void);

/* A context owns one HIP device, a stream and device workspaces. */
int dg_ctx_create(int device, dg_ctx **out);
void dg_ctx_destroy(dg_ctx *ctx);
/* The context's HIP stream (hipStream_t), for callers that order their own work. */
void *dg_ctx_stream(dg_ctx *ctx);
/* Diagnostics (no reference counterpart): messages the kernel's fast path
 * handed to the exact machine, and messages redone with the 4096-deep stack,
 * summed over this context's launches since the last reset. Synchronizes the
 * device. */
int dg_ctx_stats(dg_ctx *ctx, uint64_t *bails, uint64_t *deeps, int reset);

/* Diagnostics: the context's n (<= 16) raw device counters: [0] bails, [1]
 * deep redos, [2..11] wave-kernel phase cycles in a -DDG_WPROF build, [12]
 * messages the deep passes of dg_kids_* reran (count and emit pass each). */
int dg_ctx_counters(dg_ctx *ctx, uint64_t *out, int n, int reset);

/* Routing knobs (no reference counterpart; testing and tuning). They are read
 * from the environment ONCE, by dg_ctx_create, and changed only through these
 * calls, so routing never changes under a running launch:
 *   "flat"        DG_FLAT         -1 auto, 0 never, 1 always the flat kernel for flat roots
 *   "wave_min"    DG_WAVE_MIN     messages longer than this go to the wave kernel (512)
 *   "wave_occ"    DG_WAVE_OCC     0 auto, 4 or 5: the wave kernel's waves/SIMD instance
 *   "small_mpw"   DG_SMALL_MPW    small-kernel messages per wave (64); 0 = lane kernel
 *   "list_blocks" DG_LIST_BLOCKS  grid of the exact-machine list pass (16)
 *   "t2j_spread"  DG_T2J_SPREAD   0 auto, 1, 2 or 4 lanes per t2j message
 *   "t2j_wave_min" DG_T2J_WAVE_MIN t2j messages longer than this take the t2j wave kernel (512; 0 never)
 *   "flat_wrap"   DG_FLAT_WRAP    -1 auto, 0 off: the flat kernel for {"key":{flat}} members of a non-flat root
 *   "tget_spread" DG_TGET_SPREAD  0 auto, 1, 2 or 4: every how-manieth lane of the path-lookup kernel takes a
 *                                 (message, path) pair
 *   "cut_wave_min" DG_CUT_WAVE_MIN messages at least this long take the wave route of the cut (4096; 0 = all)
 *   "edit_wave_min" DG_EDIT_WAVE_MIN edited messages at least this long take the wave route of the splice (4096; 0 = all)
 *   "edit_lanes"  DG_EDIT_LANES   lanes per message on the splice's lane route: 1, 4 or 16 (4)
 *                                 (both knobs route dg_edit_* and dg_editm_* alike)
 *   "kids_wide_min" DG_KIDS_WIDE_MIN a list, set or map node of fixed-size entries with at least this many children
 *                                 is emitted one lane per record (256; 0 = never)
 *   "kids_no_scan" (no env)       timing only: 1 = dg_kids_* calls leave the scan out, so d_rec_off is not written
 *                                 (tools/kids_bench.py times the count pass alone with it, without d_recs)
 *   "cols_full_search" (no env)   timing only: 1 = every lane of dg_cols_list_device's emit searches all n offsets
 *                                 for its message (0: between the answers of its block's first and last lane)
 *   "ents_stage"  (no env)        dg_ents_emit_device's variable-stride emit: 4, 8 or 16 = a lane stages that many
 *                                 entries in LDS a round and its wave writes them out in runs (16); 0, and anything
 *                                 else: every lane stores its entries itself
 *   "vals_lane_emit" (no env)     1 = dg_vals_* writes every cell, string payloads and list elements included, by the
 *                                 one lane that owns it (0: a head pass and a wave-parallel body pass)
 *   "edit_reuse_rec" (no env)     timing only: 1 = a dg_edit_* or dg_editm_* launch of as many messages and items as
 *                                 the context's previous one skips the lookup and splices from its records
 *                                 (tools/edit_bench.py times the splice alone with it; another batch or other
 *                                 paths give undefined results)
 * Unknown names return DG_E_INVALID. Thread-safe (the context lock). */
int dg_ctx_set_knob(dg_ctx *ctx, const char *name, int64_t value);
int dg_ctx_get_knob(dg_ctx *ctx, const char *name, int64_t *value);

/* Upload a dg_desc blob (v1 or v2) (include/dgj2t_desc.h) to the context's device.
 * Replaces reading the Go *thrift.TypeDescriptor graph in place
 * (native/thrift.h:70-137 <-> thrift/descriptor.go:119-267). */
int dg_desc_create(dg_ctx *ctx, const void *blob, size_t len, dg_desc **out);
/* Same, for a blob already resident in device memory (e.g. received by an
 * RCCL broadcast on a non-root rank). */
int dg_desc_create_device(dg_ctx *ctx, const void *d_blob, size_t len, dg_desc **out);
void dg_desc_destroy(dg_desc *desc);
/* Root type index recorded in the blob header. */
uint32_t dg_desc_root(const dg_desc *desc);

/*
 * Device-resident batch: every pointer is device memory of ctx's device.
 *   d_json      JSON arena (at least in_off[n] + 16 readable bytes)
 *   d_in_off    n+1 u64 offsets into d_json; message i = [in_off[i], in_off[i+1])
 *   d_out       output arena; message i may use [out_off[i], out_off[i+1])
 *   d_out_off   n+1 u64 slot bounds (e.g. prefix sum of dg_slot_bound(len)).
 *               A slot may start at any byte and have any size, 0 included:
 *               the kernels write [out_off[i], out_off[i+1]) and nothing else
 *               (the wave and flat kernels' writers store the partial words
 *               at both ends of what they own byte-exactly; the lane writer
 *               stores whole words only at an 8-aligned base and bytes
 *               otherwise). 8-aligned bases are the fast case, not a
 *               requirement.
 *   d_out_len   n u32: Thrift bytes written for message i (0 on error; for
 *               DG_ST_OUT_OVERFLOW: the bytes the message needs)
 *   d_ret       n u64: packed reference status (0 = ok), or DG_ST_OUT_OVERFLOW
 *   d_pending   optional u32 counter (device), incremented once per message
 *               left with DG_ST_OUT_OVERFLOW; may be NULL
 * Enqueued on ctx's stream (or `stream` if non-NULL); asynchronous. ctx's
 * stream is a blocking stream, so it is ordered with the legacy default
 * stream (handle 0) both ways. Launches
 * on different streams of one context may run concurrently: each stream gets
 * its own device scratch (lists, counters, workspaces), up to 40 streams per
 * context (an aggregator's ring of up to 24, the in-flight and pipeline
 * streams); beyond that a shared scratch orders the launches with events, so
 * launches on streams that share one run one after the other.
 * Equivalent, per message, to BinaryConv.Do(ctx, desc, jbytes)
 * (conv/j2t/conv.go:53-77) with the given flags.
 */
int dg_j2t_batch_device(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *d_json,
                        const uint64_t *d_in_off, uint64_t n, uint64_t flags, uint8_t *d_out,
                        const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret,
                        uint32_t *d_pending, void *stream);

/* The same with the batch's longest message length (0 = unknown). The host
 * that built the arena knows it for free; with it the library schedules only
 * the kernels the batch needs (all messages short: the lane kernel alone,
 * no wave-kernel / exact-list launches). */
int dg_j2t_batch_device_ml(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *d_json,
                           const uint64_t *d_in_off, uint64_t n, uint64_t flags, uint8_t *d_out,
                           const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret,
                           uint32_t *d_pending, void *stream, uint64_t max_len);

/* dg_j2t_batch_device_ml for DG_F_HM_SPLIT batches (HTTPConv with the host
 * half of the reference's HTTP-mapping callbacks): d_hm_tab holds n_hm
 * dg_hm_entry per message (dgj2t_defs.h), the bytes handleHttpMappings
 * (conv/j2t/impl.go:243-292) wrote for each struct with mapped fields and the
 * mask of the fields it wrote, into d_hm_bytes. Where the reference returns
 * ERR_HM to Go, the kernel writes the entry's bytes and resumes. A ROOT whose
 * unset fields go to the reference's field cache (F_TRACE_BACK) comes back as
 * DG_ST_HM_END for the host to finish; DG_ST_HM_ERR = the host's entry was an
 * error. d_hm_tab NULL = the root's mapped fields only, all written by the
 * host (its bytes put in front by the caller). */
int dg_j2t_batch_device_hm(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *d_json,
                           const uint64_t *d_in_off, uint64_t n, uint64_t flags, const dg_hm_entry *d_hm_tab,
                           uint32_t n_hm, const uint8_t *d_hm_bytes, uint8_t *d_out, const uint64_t *d_out_off,
                           uint32_t *d_out_len, uint64_t *d_ret, uint32_t *d_pending, void *stream,
                           uint64_t max_len);

/* dg_j2t_batch_device_ml with the host's answers to the reference's Go
 * callbacks (dg_cb_tables, dgj2t_defs.h; device pointers): the HTTP-mapping
 * table of dg_j2t_batch_device_hm and the value-mapping answers (ERR_VM_END,
 * handleValueMapping conv/j2t/impl_amd64.go:117-155). cb NULL = none. */
int dg_j2t_batch_device_cb(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *d_json,
                           const uint64_t *d_in_off, uint64_t n, uint64_t flags, const dg_cb_tables *cb,
                           uint8_t *d_out, const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret,
                           uint32_t *d_pending, void *stream, uint64_t max_len);

/* dg_j2t_batch_device_ml enqueued `iters` times back to back in one call
 * (one lock, no host round trip between batches): a host that re-runs the
 * same job -- benchmarks, replays -- keeps the GPU fed. Every iteration is a
 * complete conversion of the batch. */
int dg_j2t_batch_device_iters(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *d_json,
                              const uint64_t *d_in_off, uint64_t n, uint64_t flags, uint8_t *d_out,
                              const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret,
                              uint32_t *d_pending, void *stream, uint64_t max_len, int iters);

/* dg_j2t_batch_device_iters with HIP timing events around each of the batch's
 * launches (measurement only: the events add a few microseconds between
 * kernels). ms[0] = the first kernel (flat, small or lane), ms[1] = the wave
 * kernel, ms[2] = the list pass (exact machine), each averaged over `iters`
 * serial conversions; 0 for a launch the route does not make. Returns after
 * the stream has drained. */
int dg_j2t_batch_device_ktime(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *d_json,
                              const uint64_t *d_in_off, uint64_t n, uint64_t flags, uint8_t *d_out,
                              const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret,
                              uint32_t *d_pending, void *stream, uint64_t max_len, int iters, double *ms);

/* One in-flight batch's outputs (dg_j2t_batch_device_inflight). */
typedef struct dg_out_set {
    uint8_t *d_out;      /* slot arena, laid out by the shared d_out_off */
    uint32_t *d_out_len;
    uint64_t *d_ret;
    uint32_t *d_pending;
} dg_out_set;

/* `iters` complete conversions of the batch with up to `depth` (1..8) of them
 * in flight at once: conversion k writes sets[k % depth] on the context's
 * k % depth-th stream (stream 0 = `stream`; the others are the context's own,
 * forked from `stream` at the call and joined back into it before return, so
 * work enqueued on `stream` afterwards sees every conversion done). Batch k+1's
 * kernels fill the CUs batch k's tail and list pass leave idle -- what a
 * gateway with several batches from its aggregator in flight runs. depth 1 is
 * dg_j2t_batch_device_iters. */
int dg_j2t_batch_device_inflight(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *d_json,
                                 const uint64_t *d_in_off, uint64_t n, uint64_t flags, const uint64_t *d_out_off,
                                 const dg_out_set *sets, int depth, void *stream, uint64_t max_len, int iters);

/* Output-slot size the device path uses by default for a message of len
 * bytes: 4 len + 64 rounded up to 128 (slots on L2-line boundaries: a line
 * written in part is written back whole). */
uint64_t dg_slot_bound(uint64_t len);

/*
 * Host batch (pinned or pageable host memory): H2D, kernels, overflow reruns,
 * D2H with the outputs compacted. On return out holds the n outputs back to
 * back: message i is out[out_off[i], out_off[i+1]) (empty on error, see ret).
 * out_cap must be >= the total; *out_need receives the total required (if the
 * call returns DG_E_NOMEM because out_cap was too small, retry with it).
 */
int dg_j2t_batch_host(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *json,
                      const uint64_t *in_off, uint64_t n, uint64_t flags, uint8_t *out, uint64_t out_cap,
                      uint64_t *out_off, uint64_t *ret, uint64_t *out_need);

/* dg_j2t_batch_host with the HTTP-mapping table of dg_j2t_batch_device_hm
 * (host memory; hm_bytes of hm_len bytes). DG_ST_HM_END messages keep their
 * partial output (and requires words) in out. */
int dg_j2t_batch_host_hm(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *json,
                         const uint64_t *in_off, uint64_t n, uint64_t flags, const dg_hm_entry *hm_tab, uint32_t n_hm,
                         const uint8_t *hm_bytes, uint64_t hm_len, uint8_t *out, uint64_t out_cap, uint64_t *out_off,
                         uint64_t *ret, uint64_t *out_need);

/* dg_j2t_batch_host with the host's callback answers (dg_cb_tables, host
 * memory): DG_ST_HM_END messages keep their partial output (and requires
 * words) in out, ERR_VM_END messages (code 24) their 16-byte record. */
int dg_j2t_batch_host_cb(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *json,
                         const uint64_t *in_off, uint64_t n, uint64_t flags, const dg_cb_tables *cb, uint8_t *out,
                         uint64_t out_cap, uint64_t *out_off, uint64_t *ret, uint64_t *out_need);

/* One message, BinaryConv.Do semantics (conv/j2t/conv.go:53-77). *out_len is
 * the Thrift length; returns the packed status word through *ret. */
int dg_j2t_do(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *json, size_t len,
              uint64_t flags, uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *ret);

/* Pack the converted messages for the device->host copy: message i's
 * d_out_len[i] bytes move from its slot (d_out + d_out_off[i]) to
 * d_dst + d_dst_off[i], where d_dst_off is the exclusive prefix sum of
 * d_out_len (caller-computed, e.g. one scan kernel). Stream-ordered; errored
 * messages have out_len 0. The Go side then hands (dst, dst_off) to the NIC
 * path without per-message copies. */
int dg_pack_device(dg_ctx *ctx, const uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_len, uint64_t n,
                   uint8_t *d_dst, const uint64_t *d_dst_off, void *stream);

/* dg_pack_device with the prefix sum folded in (one launch): computes
 * d_dst_off[0..n] = exclusive prefix sum of d_out_len (d_dst_off[n] = total
 * bytes) and packs message i's bytes at d_dst + d_dst_off[i]. Stream-ordered
 * after the conversion that wrote d_out_len. */
int dg_pack_device_scan(dg_ctx *ctx, const uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_len,
                        uint64_t n, uint8_t *d_dst, uint64_t *d_dst_off, void *stream);

/* HTTPConv framing (conv/j2t/http_conv.go:68-114) fused into the packing:
 * every message that converted (d_ret[i] == 0) is packed as
 * hdr + body + ftr, every failed one as nothing; d_dst_off as in
 * dg_pack_device_scan. hdr/ftr are host bytes (the message header and footer
 * of thrift.GetBinaryMessageHeaderAndFooter, thrift/binary.go:137-175),
 * copied by the call; (hdr_len rounded up to 8) + ftr_len must be <= 4080. */
int dg_pack_device_framed(dg_ctx *ctx, const uint8_t *d_out, const uint64_t *d_out_off, const uint32_t *d_out_len,
                          const uint64_t *d_ret, uint64_t n, const uint8_t *hdr, uint32_t hdr_len, const uint8_t *ftr,
                          uint32_t ftr_len, uint8_t *d_dst, uint64_t *d_dst_off, void *stream);

/*
 * Batching aggregator: concurrent single-message calls coalesced into device
 * batches (the reference's callers run BinaryConv.Do from many goroutines,
 * conv/j2t/conv_timing_test.go:76-99). dg_agg_do blocks the calling thread
 * until its message is converted, with the semantics of dg_j2t_do
 * (BinaryConv.Do, conv/j2t/conv.go:53-77); see dg_agg_create2 for when a
 * batch is converted. If out_cap is too small the call returns
 * DG_E_NOMEM with *out_len = the bytes needed. Thread-safe.
 */
int dg_agg_create(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, uint64_t flags, uint32_t max_batch,
                  uint32_t max_wait_us, dg_agg **out);
int dg_agg_do(dg_agg *agg, const uint8_t *json, size_t len, uint8_t *out, size_t out_cap, size_t *out_len,
              uint64_t *ret);
/* dg_agg_create with an explicit JSON capacity. Capacities are per caller
 * thread: every thread that calls owns a part of each device batch holding
 * up to max_batch messages and max_bytes JSON bytes (a message longer than
 * max_bytes is converted alone); a batch is sealed when one thread's part is
 * full, when a caller waits on it, or when its first message has waited
 * max_wait_us. dg_agg_create uses max_bytes = max(1 MiB, 512 B x max_batch).
 * The first 224 calling threads get a part each; further threads share the
 * last 32 parts under a per-part lock (no thread count converts alone).
 * Pinned host memory: every part that is in use holds ring x (8 x max_batch +
 * max_bytes + 64) bytes (ring = DG_AGG_RING, default 16, at most 24), e.g. 16
 * threads x 16 x (8 x 4096 + 2 MiB) = 520 MiB. On top of that, every batch
 * of the ring keeps buffers for the largest batch the registered parts can
 * make, P = 4 x (parts x max_bytes) + 128 x (parts x max_batch) bytes of
 * packed output: about P of pinned host memory and 5 P of device memory per
 * batch, ring x that in all. They are sized exactly (never regrown mid-run)
 * while ring x P <= 4 GiB (knob "exact_total"), else grown lazily to twice
 * the batch that needed them. E.g. 16 threads, max_batch 4096, max_bytes
 * 1 MiB: P = 72 MiB, ring 16: 1.15 GiB pinned + 5.8 GiB device. Size
 * max_batch / max_bytes for the caller threads the process runs. */
int dg_agg_create2(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, uint64_t flags, uint32_t max_batch,
                   uint64_t max_bytes, uint32_t max_wait_us, dg_agg **out);
/* Asynchronous form of dg_agg_do, for a caller with many requests in flight
 * (an event loop, or a goroutine pool behind one OS thread): dg_agg_submit
 * copies the JSON into the open batch and returns a ticket; dg_agg_wait
 * blocks until the ticket's batch is converted and copies its result out
 * (same results as dg_agg_do). Every ticket must be waited for exactly once,
 * and `json` must stay valid until then. With nonblock, dg_agg_submit
 * returns DG_E_AGAIN instead of blocking when no batch is open (a caller
 * that holds unwaited tickets must use it, and wait for its oldest ticket
 * before retrying: the next batch opens when the oldest one's callers have
 * taken their results). */
typedef struct dg_agg_ticket {
    void *batch;
    uint64_t gen;
    uint32_t idx;
    const uint8_t *json;
    size_t len;
} dg_agg_ticket;
int dg_agg_submit(dg_agg *agg, const uint8_t *json, size_t len, int nonblock, dg_agg_ticket *t);
int dg_agg_wait(dg_agg *agg, dg_agg_ticket *t, uint8_t *out, size_t out_cap, size_t *out_len, uint64_t *ret);
/* 1 when dg_agg_wait on the ticket would not block (its batch is converted),
 * else 0: an event loop takes its completions as they come. */
int dg_agg_ready(dg_agg *agg, const dg_agg_ticket *t);
/* batches flushed and messages converted so far */
int dg_agg_stats(dg_agg *agg, uint64_t *batches, uint64_t *msgs);
/* diagnostics: n <= 16 summed counters (ns unless noted) (flusher waiting for a seal,
 * for a free batch, issuing a batch; completer waiting for the header, for
 * the packed bytes; seal to issued; issued to done; callers blocked in
 * dg_agg_wait; dg_agg_drive: time in submit, in wait, and the count of
 * submits that met no open batch; the count of calls converted alone by
 * dg_j2t_do: longer than a part, or no part left for their thread; the
 * flusher's issue split in four: waiting for the parts' writers, buffers,
 * the gather launch, the conversion's launches).
 * An exclusive part (one of 224) belongs to a calling thread from its first
 * call until the thread exits; an exited thread's part goes to the next new
 * thread. */
int dg_agg_profile(dg_agg *agg, uint64_t *out, int n);
/* converts what is still queued, then stops the flusher (every ticket must
 * have been waited for) */
void dg_agg_destroy(dg_agg *agg);
/* Benchmark driver (the reference's b.RunParallel over Do,
 * conv/j2t/conv_timing_test.go:76-99): `threads` OS threads each convert a
 * contiguous share of the n messages through the aggregator with up to
 * `window` requests in flight, message i's result into
 * out[out_off[i] .. out_off[i+1]) with out_len[i], ret[i], and, if lat_ns,
 * its submit-to-result latency for every 8th message (0 for the others: the
 * clock is read for a sample of the calls only). *seconds = wall time of
 * the whole run. */
int dg_agg_drive(dg_agg *agg, const uint8_t *arena, const uint64_t *in_off, uint64_t n, int threads, int window,
                 uint8_t *out, const uint64_t *out_off, uint64_t *out_len, uint64_t *ret, uint32_t *lat_ns,
                 double *seconds);

/* The gateway binding: goroutines do not hold an OS
 * thread while their call converts. A Do submits without blocking
 * (dg_agg_submit nonblock), takes the ticket's generation
 * (dg_agg_ticket_gen) and parks on a Go channel for it; ONE poller thread
 * blocks in dg_agg_wait_gen, which returns once batches up to a newer
 * generation are converted (generations complete in order), and wakes the
 * goroutines of every generation up to it; each then calls dg_agg_wait,
 * which no longer blocks, to copy its result. Every ticket must be waited
 * for, from any thread. */
int dg_agg_wait_gen(dg_agg *agg, uint64_t after, uint32_t timeout_us, uint64_t *done);
uint64_t dg_agg_ticket_gen(const dg_agg_ticket *t);
/* aggregator knobs: "depth" (0 = off): also seal the open batch as soon as
 * it holds a message and fewer than depth batches are converting -- for
 * callers that park instead of blocking in dg_agg_wait, whose waits the
 * aggregator cannot see; "min_fill" (0 = off): the depth rule seals only a
 * batch of at least this many calls (many parked callers refill a batch
 * over a round trip: sealing at once keeps batches small); "max_wait_us":
 * the seal timer of dg_agg_create; "exact_total" (bytes, default 4 GiB):
 * the ring-wide budget for sizing batch buffers exactly (dg_agg_create2). */
int dg_agg_set_knob(dg_agg *agg, const char *name, int64_t value);
/* Benchmark driver for the gateway shape: `callers` logical callers, each
 * with ONE call in flight at a time (a goroutine in Do), multiplexed over
 * `workers` OS threads (the Go runtime's Ms) with the dg_agg_wait_gen poller
 * above; worker w serves messages [w n / workers, (w + 1) n / workers) in
 * order, each runnable caller taking the next one (workers is clamped to
 * min(workers, callers, n): a worker needs callers for its range). Outputs as
 * dg_agg_drive; stats (optional, 8 u64): parks, submits retried for want of
 * room, poller wake-ups, callers, then ns summed over the workers in
 * dg_agg_wait, in dg_agg_submit, idle, and in all. */
int dg_agg_gateway_drive(dg_agg *agg, const uint8_t *arena, const uint64_t *in_off, uint64_t n, int workers,
                         int callers, uint8_t *out, const uint64_t *out_off, uint64_t *out_len, uint64_t *ret,
                         uint32_t *lat_ns, double *seconds, uint64_t *stats);

/* dg_j2t_batch_host for large host batches: the batch is streamed in
 * `chunks` pieces through 3 stream-private buffer sets, so the upload of
 * chunk k+1, the kernels of chunk k and the download of chunk k-1 overlap,
 * all issued from C. json, in_off, out, out_off and ret should be pinned
 * (hipHostMalloc) for the copies to be asynchronous. Same outputs and
 * DG_E_NOMEM/out_need contract as dg_j2t_batch_host; json needs no padding. */
int dg_j2t_pipeline_host(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *json,
                         const uint64_t *in_off, uint64_t n, uint64_t flags, uint32_t chunks, uint8_t *out,
                         uint64_t out_cap, uint64_t *out_off, uint64_t *ret, uint64_t *out_need);

/*
 * t2j: Thrift binary -> JSON (the reverse path, conv/t2j). Replaces
 * BinaryConv.Do / DoInto (conv/t2j/conv.go:50-95 over impl.go:74-468) for
 * the options in dgj2t_defs.h DG_T2J_* (the Go-side ones -- HTTP mapping,
 * ConvertException, EnableThriftBase -- stay on the Go host).
 *
 * dg_desc_attach_t2j uploads the descriptor's t2j side table (the JSON key
 * text per field, include/dgj2t_desc.h dg_t2j_*) once; the t2j entry points
 * need it. Status words: 0, DG_T2J_E_* | pos << 8 | value << 40 (pos = the
 * Thrift read offset), or DG_ST_OUT_OVERFLOW with *out_len = bytes needed
 * (device entry point only; the host entry point reruns those itself).
 * Nesting deeper than the fast kernel's LDS frames is rerun on device with
 * 4096 frames per message; deeper still is DG_T2J_E_DEPTH.
 */
int dg_desc_attach_t2j(dg_desc *desc, const void *side, size_t len);
/* the slot size the host entry point gives a message of len Thrift bytes:
 * 3 len + 64 rounded up to 128 (a guess: JSON has no fixed bound over Thrift;
 * larger outputs overflow and are rerun with their exact size) */
uint64_t dg_t2j_slot_bound(uint64_t len);
/* device buffers, stream-ordered, async; arena readable 16 bytes past the
 * last message; d_out_off 8-aligned slots */
int dg_t2j_batch_device(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *d_thrift,
                        const uint64_t *d_in_off, uint64_t n, uint64_t opts, uint8_t *d_out,
                        const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret, void *stream);
/* The same with the batch's longest Thrift message (0 = unknown): the kernel
 * gives short messages full waves and ~1 KB ones sparse waves (t2j-c2 +4 %,
 * t2j-c3 +5 % over the size-blind launch). */
int dg_t2j_batch_device_ml(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *d_thrift,
                           const uint64_t *d_in_off, uint64_t n, uint64_t opts, uint8_t *d_out,
                           const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret, void *stream,
                           uint64_t max_len);
/* host buffers, synchronous: JSON packed back to back into out (out_off[n+1]);
 * DG_E_NOMEM with *out_need when out_cap is too small */
int dg_t2j_batch_host(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *thrift,
                      const uint64_t *in_off, uint64_t n, uint64_t opts, uint8_t *out, uint64_t out_cap,
                      uint64_t *out_off, uint64_t *ret, uint64_t *out_need);

/* dg_t2j_batch_device_ml / dg_t2j_batch_host with the device part of the Go-side options
 * device part (dgj2t_defs.h DG_T2J_CONVERT_EXC, DG_T2J_SKIP_RESP_BASE): aux
 * (n u64, device resp. host memory) receives each message's response-base
 * span when DG_T2J_SKIP_RESP_BASE is set (may be NULL otherwise); a
 * DG_T2J_E_EXCEPTION message keeps its JSON in out. */
int dg_t2j_batch_device_aux(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *d_thrift,
                            const uint64_t *d_in_off, uint64_t n, uint64_t opts, uint8_t *d_out,
                            const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret, uint64_t *d_aux,
                            void *stream, uint64_t max_len);
int dg_t2j_batch_host_aux(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *thrift,
                          const uint64_t *in_off, uint64_t n, uint64_t opts, uint8_t *out, uint64_t out_cap,
                          uint64_t *out_off, uint64_t *ret, uint64_t *out_need, uint64_t *aux);
/* ... and EnableHttpMapping's response side (DG_T2J_HM; conv/t2j/impl.go:
 * 132-142, 296-306, writeHttpValue 515-588; HandleRequires' mapped unsets):
 * a mapped field of the root struct or of a struct that is a root field's
 * value stops the message with DG_T2J_E_CALLBACK and a 16-byte record in out
 * (dgj2t_defs.h). The host runs writeHttpValue (dynamicgo_amd/t2j.py) and
 * converts the message again with its answers: ans_tab (n entries, device
 * resp. host memory) indexes one byte per answer in the answer bytes, consumed
 * in the order the stops come. cb: only ans_tab, bytes and len are read. */
int dg_t2j_batch_device_cb(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *d_thrift,
                           const uint64_t *d_in_off, uint64_t n, uint64_t opts, uint8_t *d_out,
                           const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret, uint64_t *d_aux,
                           const dg_cb_entry *d_ans, const uint8_t *d_ans_bytes, void *stream, uint64_t max_len);
int dg_t2j_batch_host_cb(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *thrift,
                         const uint64_t *in_off, uint64_t n, uint64_t opts, uint8_t *out, uint64_t out_cap,
                         uint64_t *out_off, uint64_t *ret, uint64_t *out_need, uint64_t *aux, const dg_cb_tables *cb);

/*
 * tget: batched GetByPath over Thrift-binary messages (the reference's
 * thrift/generic Node.GetByPath / Value.GetByPath, node.go:292-484 and
 * value.go:70-161): the byte span of a sub-value, found by walking field
 * headers and skipping values, nothing else decoded. A path set (1 to
 * DG_TGET_MAX_PATHS paths of up to DG_TGET_MAX_STEPS steps, blob layout in
 * dgj2t_defs.h under DG_PATH_MAGIC) is validated and uploaded once, then
 * evaluated for every message of a batch in one launch.
 *
 * The create call returns DG_E_ARG (text in dg_last_error) for a blob that
 * breaks a limit: no path or more than 8, more than 16 steps in a path, an
 * unknown step kind, a field id outside int16, a negative index, a key outside
 * the pool, a table outside the blob. A path set belongs to its context and is
 * read-only after creation (any number of launches may share it); destroy it
 * only after the launches that use it have finished.
 */
typedef struct dg_path dg_path;
int dg_path_create(dg_ctx *ctx, const void *blob, size_t len, dg_path **out);
void dg_path_destroy(dg_path *p);
uint32_t dg_path_count(const dg_path *p);

/* One result: path k on message i is rec[i * P + k], P = the set's path
 * count. Offsets are relative to the message's first byte (messages of 4 GiB
 * or more are DG_TGET_E_READ, aux = 0xFFFFFFFF). By status (dgj2t_defs.h):
 *   DG_TGET_OK         [start, end) = the sub-value, type = its wire type
 *                      (the field header's, or the container header's element
 *                      type; root_type for the empty path, whose span is the
 *                      whole top value); step = the path length; aux = 0.
 *   DG_TGET_NOT_FOUND  step = the step that missed; end = start; a FIELD step:
 *                      type STRUCT, start 0; an INDEX step: type LIST or SET,
 *                      start = the offset after the list header; a key step:
 *                      type MAP, start = the offset after the map header.
 *                      aux = the read offset at the miss (after the STOP byte,
 *                      the list header, or the map's last entry).
 *                      LIST and SET share one wire form: type is LIST when the
 *                      wire type of the last field header the path went
 *                      through (root_type when it went through none) is LIST,
 *                      else SET. This is Value.GetByPath's rule (value.go:122,
 *                      131); Node.GetByPath tests the ROOT node's type at every
 *                      field step (node.go:456, a slip) and is not followed.
 *   DG_TGET_E_READ     meta.ErrRead: a short buffer, an invalid wire type in a
 *                      field, list or map header, a negative container size, a
 *                      negative or over-long string size, skip depth beyond
 *                      1023. step = the step that failed, the path length for
 *                      the final skip; start = end = type = aux = 0.
 *   DG_TGET_E_TYPE     meta.ErrDismatchType: a STRKEY step on a map whose key
 *                      type is not STRING, an INTKEY step on one whose key
 *                      type is not I08, I16, I32 or I64. step = that step, aux
 *                      = the map's key type; start = end = type = 0.
 * A step applied to a value of another shape (INDEX on a struct, ...) is no
 * error in the reference: the bytes are read as the header the step expects,
 * and so here. An INTKEY on an I08-keyed map compares the key byte UNSIGNED
 * (ReadInt returns int(byte), thrift/binary.go:739-741): -1 never hits, 255
 * hits the byte 0xFF. */
typedef struct dg_tget_rec {
    uint32_t start, end;
    uint8_t type, status;
    uint16_t step;
    uint32_t aux;
} dg_tget_rec; /* 16 bytes */

/* Device buffers, stream-ordered, async (stream NULL: the context's). Message
 * i is d_thrift[d_in_off[i], d_in_off[i+1]); no byte past d_in_off[i+1] counts
 * as part of it. The arena is readable 16 bytes past its last message.
 * root_type: the wire type of each message's top value (12 = STRUCT as a rule;
 * LIST, SET and MAP roots are legal). d_rec: n * P records, 16-byte aligned
 * (each is one 16-byte store). d_val_off (u64)
 * and d_val_len (u32), n * P entries each, may be NULL: they receive
 * d_in_off[i] + start and end - start (length 0 unless DG_TGET_OK), the
 * (slot offset, length) arrays dg_pack_device_scan takes to pack the found
 * values of a P = 1 run back to back. max_len: the batch's longest message
 * (0 = unknown), a hint for the lane spacing (dense lanes measured fastest at
 * ~100 B and at ~1.2 KB, so every length takes them today; the tget_spread
 * knob forces another). n = 0 returns DG_OK and launches
 * nothing; n * P must stay below 2^32. A value nested deeper than the kernel's
 * 8 LDS skip frames is rerun on device with 1024 frames in device memory;
 * past 1023 levels the reference fails too (DG_TGET_E_READ). */
int dg_tget_batch_device(dg_ctx *ctx, const dg_path *paths, uint8_t root_type, const uint8_t *d_thrift,
                         const uint64_t *d_in_off, uint64_t n, dg_tget_rec *d_rec, uint64_t *d_val_off,
                         uint32_t *d_val_len, void *stream, uint64_t max_len);
/* Host buffers, synchronous: thrift[in_off[i], in_off[i+1]), rec n * P. */
int dg_tget_batch_host(dg_ctx *ctx, const dg_path *paths, uint8_t root_type, const uint8_t *thrift,
                       const uint64_t *in_off, uint64_t n, dg_tget_rec *rec);

/*
 * cut: batched MarshalTo ("cutting", the reference's thrift/generic
 * Value.MarshalTo, value.go:375-552): every message, written under a wide
 * descriptor `from`, is re-emitted under a narrower descriptor `to`. Fields
 * `to` does not know are dropped at every nesting level, the requiredness of
 * `to` is enforced, and under DG_CUT_WRITE_DEFAULT the unset default fields of
 * `to` are written as empty values. A plan (the pair graph compiled by
 * generic.compile_cut, blob layout in dgj2t_defs.h under DG_CUT_MAGIC) is
 * validated and uploaded once (DG_E_ARG, text in dg_last_error, for a blob
 * that breaks the layout), belongs to its context and is read-only after.
 *
 * Per message, d_ret[i] = status (bits 0-7) | aux << 32 and d_out_len[i]:
 *   DG_CUT_OK          out_len bytes in the slot
 *   DG_CUT_E_READ      meta.ErrRead: a short buffer, an invalid type byte in a
 *                      field, list or map header, a negative size, skip depth
 *                      beyond 1023 (a message of 4 GiB or more: aux 0xFFFFFFFF)
 *   DG_CUT_E_TYPE      meta.ErrDismatchType: a field whose wire type is not the
 *                      one `from` declares (aux = the field id), or a value
 *                      whose `from` and `to` types cannot be cut (aux = 0)
 *   DG_CUT_E_UNKNOWN   meta.ErrUnknownField under DG_CUT_DISALLOW_UNKNOWN, aux
 *                      = the field id
 *   DG_CUT_E_REQUIRED  meta.ErrMissRequiredField, aux = the lowest missing id
 *   DG_CUT_E_OVERFLOW  the slot is too small; out_len = aux = the bytes needed
 *                      (saturated at 2^32 - 1)
 *   DG_CUT_E_DEPTH     more than DG_CUT_MAX_DEPTH cut containers open
 * Field ids in aux are sign-extended to 32 bits. out_len is 0 for every error
 * but the overflow: the reference returns no bytes on error.
 *
 * Deviations from the reference, all stated by generic.compile_cut too: the
 * same struct descriptor on both sides (value.go:395-397 returns without
 * reading, which desynchronises its reader) and a `to` struct against a `from`
 * that is none (a nil dereference there) are refused when the plan is
 * compiled; a `to` struct with more than 64 tracked fields is refused (one
 * mask word per frame); the reference recurses without limit where
 * DG_CUT_E_DEPTH ends a message (the depth inside a skipped or copied value is
 * not counted: it keeps SkipType's 1023).
 *
 * Memory contract. Message i is d_thrift[d_in_off[i], d_in_off[i+1]); the arena
 * is readable 16 bytes past its last message. Its slot is d_out[d_out_off[i],
 * d_out_off[i+1]) at any alignment: no byte outside it is written, and on
 * success no byte at or beyond d_out_off[i] + out_len (neither route rounds a
 * store up). A message that fails or overflows may leave bytes anywhere in its
 * own slot. d_out must not alias the input.
 *
 * Two routes in one launch sequence: a lane per message (short messages), and
 * a wave per message for those at least "cut_wave_min" bytes long or nested
 * beyond the lane route's 8 frames, queued on the device.
 */
typedef struct dg_cut dg_cut;
int dg_cut_create(dg_ctx *ctx, const void *blob, size_t len, dg_cut **out);
void dg_cut_destroy(dg_cut *p);
/* The slot size that can never overflow for a message of len bytes: len when
 * no literal can be written (no DG_CUT_WRITE_DEFAULT, or DG_CUT_NOT_CHECK_REQ,
 * or a plan without default fields), else len * (1 + U), U = the plan's
 * largest per-struct literal total (every struct instance costs at least its
 * STOP byte and adds at most U). A worst case: callers may give less and
 * rerun the messages that report DG_CUT_E_OVERFLOW, as dg_cut_batch_host does. */
uint64_t dg_cut_slot_bound(const dg_cut *p, uint64_t len, uint64_t opts);
/* Device buffers, stream-ordered, async (stream NULL: the context's). opts:
 * DG_CUT_* bits. max_len: the batch's longest message (0 = unknown), a hint.
 * n = 0 returns DG_OK and launches nothing. */
int dg_cut_batch_device(dg_ctx *ctx, const dg_cut *plan, uint64_t opts, const uint8_t *d_thrift,
                        const uint64_t *d_in_off, uint64_t n, uint8_t *d_out, const uint64_t *d_out_off,
                        uint32_t *d_out_len, uint64_t *d_ret, void *stream, uint64_t max_len);
/* Host buffers, synchronous: message i's bytes at out + out_off[i] (out_off
 * has n + 1 entries; failed messages are empty, ret[i] says why); *out_need =
 * the total. Slot overflows are rerun once in exact-size slots. DG_E_NOMEM when
 * out_cap is too small (*out_need is set). */
int dg_cut_batch_host(dg_ctx *ctx, const dg_cut *plan, uint64_t opts, const uint8_t *thrift, const uint64_t *in_off,
                      uint64_t n, uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint64_t *ret,
                      uint64_t *out_need);

/*
 * edit: batched SetByPath / UnsetByPath over Thrift-binary messages (the
 * reference's thrift/generic Value.SetByPath / Node.SetByPath with setNotFound
 * and replace, value.go:263-299 and node.go:825-920, and UnsetByPath with
 * deleteChild, value.go:302-333 and node.go:1009-1127). One edit is ONE path of
 * 1 to DG_TGET_MAX_STEPS steps and one op, applied to every message of a batch:
 * the path lookup (dg_tget_*) runs on the path without its last step (`parent`)
 * and on the whole path (`full`), then a splice kernel re-emits each message as
 * prefix + new bytes + suffix with the container's count patched.
 *
 * DG_EDIT_SET (a value of wire type val_type, its bytes taken as given):
 *   full found          its type must be val_type (else DG_EDIT_E_TYPE, aux =
 *                       the type found); out = msg[0, start) + value +
 *                       msg[end, len), DG_EDIT_EXISTED set.
 *   full missed at its  an insert at the FRONT of the container (the reference's
 *   last step           TestSetByPath reads the new element back at index 0):
 *                       FIELD: type(1) id(BE16) value at parent.start, the first
 *                       byte of the struct that was searched (parent must be
 *                       found: its status passes through otherwise); INDEX: value
 *                       after the list header; a key step: key bytes + value after
 *                       the map header (STRKEY: 4-byte length + bytes; BINKEY: the
 *                       pool bytes; INTKEY: the key big-endian at the width of the
 *                       map's key type). The container's big-endian i32 count gets
 *                       int32(count + 1), wrapping as the reference's does. A
 *                       val_type that is not the list's element / the map's value
 *                       type is DG_EDIT_E_TYPE (aux = the header's type).
 *   full missed earlier DG_EDIT_NOT_FOUND; DG_TGET_E_READ / DG_TGET_E_TYPE of
 *                       the lookup pass through with its aux.
 * DG_EDIT_UNSET (the value arguments are ignored):
 *   parent missed       DG_EDIT_OK, the message copied unchanged (the reference
 *                       returns nil); parent E_READ / E_TYPE pass through.
 *   parent found        a STRUCT needs a FIELD step, a LIST or SET an INDEX step,
 *                       a MAP a key step; anything else is DG_EDIT_E_TYPE (aux =
 *                       the parent's type). full found: the entry is dropped --
 *                       [start - 3, end) for a field, [start, end) for an element,
 *                       [start - key length, end) for a map entry -- the count gets
 *                       int32(count - 1) and DG_EDIT_EXISTED is set. full missed:
 *                       DG_EDIT_NOT_FOUND; full E_READ / E_TYPE pass through.
 * d_ret[i] = status | DG_EDIT_EXISTED | aux << 32; d_out_len[i] = the output
 * length, 0 on an error, the bytes needed on DG_EDIT_E_OVERFLOW (aux too,
 * saturated at 2^32 - 1). A message that fails or overflows writes nothing.
 *
 * Deviations from the reference:
 *   1. A missing field of a nested struct: searchFieldId returns start 0 on a
 *      miss (node.go:302), so SetByPath inserts the new field at byte 0 of the
 *      ROOT message whatever struct was searched; here it goes to the front of
 *      the struct that was searched.
 *   2. The key of an INTKEY insert: setNotFound encodes it with
 *      path.ToRaw(n.t), the VALUE's type (node.go:879): nil or the wrong width
 *      unless the two coincide; here the map's own key type gives the width.
 *   3. An insert into a list or map does not check the element type there and
 *      leaves a corrupt message; here a differing val_type is DG_EDIT_E_TYPE.
 *   4. Unset of an absent map key deletes the map's LAST entry there and writes
 *      count - 1 (-1 on an empty map); here it is DG_EDIT_NOT_FOUND, like the
 *      other containers.
 *   5. Keys are matched as the lookup matches them (its I08 rule included), not
 *      by deleteChild's raw compare.
 *   6. Unset on a parent that is no container silently does nothing there; here
 *      it is DG_EDIT_E_TYPE.
 *   7. The empty path (`*self = sub`) is no edit of a message: dg_edit_create
 *      refuses it with DG_E_ARG.
 * Several children of one node in one edit: dg_editm_* below (SetMany). Items
 * under different parents stay a second call on the first one's output.
 *
 * dg_edit_create takes the DG_PATH_MAGIC blob of dg_path_create with exactly
 * one path of at least one step (DG_E_ARG otherwise, and for every blob
 * dg_path_create refuses, with its texts). The handle belongs to its context
 * and is read-only after creation.
 */
typedef struct dg_edit dg_edit;
int dg_edit_create(dg_ctx *ctx, const void *path_blob, size_t len, uint32_t op, dg_edit **out);
void dg_edit_destroy(dg_edit *e);
/* The exact worst case of one message's output: DG_EDIT_UNSET: len;
 * DG_EDIT_SET: len + val_len + what the path's last step can add (FIELD 3,
 * INDEX 0, STRKEY 4 + the key's length, BINKEY the key's length, INTKEY 8). */
uint64_t dg_edit_slot_bound(const dg_edit *e, uint64_t len, uint64_t val_len);
/* Device buffers, stream-ordered, async (stream NULL: the context's). Messages
 * and root_type as dg_tget_batch_device (the arena readable 16 bytes past its
 * end; n * 2 below 2^32). Values: with d_val_off, message i's value is
 * d_val[d_val_off[i], d_val_off[i+1]) and val_len is the longest value (0 =
 * unknown), a hint; with d_val_off NULL every message gets d_val[0, val_len).
 * The value arena is readable 16 bytes past its end.
 * Message i's slot is d_out[d_out_off[i], d_out_off[i+1]) at any alignment: no
 * byte outside [d_out_off[i], d_out_off[i] + out_len) is written (no store is
 * rounded up). d_out must not alias d_thrift. max_len: the batch's longest
 * message, or 0 for unknown. The launch leaves out a route that no output can
 * take by the two hints, so a hint that is given must not be too small: a
 * message longer than it may be left unwritten. n = 0 returns DG_OK and
 * launches nothing.
 * The lookup's 2 n records live in a scratch of the context, the one dg_editm_*
 * uses, ordered across streams like the lookup's own workspace. Two routes: "edit_lanes" lanes per
 * message (1, 4 or 16), and a wave per message for outputs at least
 * "edit_wave_min" bytes long. */
int dg_edit_batch_device(dg_ctx *ctx, const dg_edit *e, uint8_t root_type, const uint8_t *d_thrift,
                         const uint64_t *d_in_off, uint64_t n, uint8_t val_type, const uint8_t *d_val,
                         const uint64_t *d_val_off, uint64_t val_len, uint8_t *d_out, const uint64_t *d_out_off,
                         uint32_t *d_out_len, uint64_t *d_ret, void *stream, uint64_t max_len);
/* Host buffers, synchronous: val / val_off as above (host memory; no spare
 * bytes needed); message i's bytes at out + out_off[i] (out_off has n + 1
 * entries; failed messages are empty, ret[i] says why); *out_need = the total.
 * Every slot has its exact bound, so nothing is rerun. DG_E_NOMEM when out_cap
 * is too small (*out_need is set). */
int dg_edit_batch_host(dg_ctx *ctx, const dg_edit *e, uint8_t root_type, const uint8_t *thrift, const uint64_t *in_off,
                       uint64_t n, uint8_t val_type, const uint8_t *val, const uint64_t *val_off, uint64_t val_len,
                       uint8_t *out, uint64_t out_cap, uint64_t *out_off, uint64_t *ret, uint64_t *out_need);

/*
 * editm: batched SetMany (the reference's Node.SetMany with getMany,
 * setNotFound per missing item and replaceMany, thrift/generic/node.go:930-1007)
 * and its UNSET counterpart. One many-edit is a parent path of 0 to
 * DG_TGET_MAX_STEPS - 1 steps, K items (1 <= K <= DG_EDITM_MAX_ITEMS), each ONE
 * last step below the parent, and one op, applied to every message of a batch:
 * what v.GetByPath(parent...).SetMany(items) gives, written back into the whole
 * message. The K last steps are of one class: all FIELD, all INDEX, or all key
 * steps (STRKEY, INTKEY and BINKEY may mix). Parent and the K full paths are one
 * path set, so one lookup launch serves all items; then one splice writes the
 * message once with all K cuts.
 *
 * DG_EDIT_SET: item j carries a value of wire type val_types[j] and is decided
 * exactly as dg_edit decides a single SET (statuses and deviations 1-7 above).
 * Found items are replaced in place; missing items are all inserted at the front
 * of the container in the order the items were given (the reference's
 * TestSetMany reads two Index(1024) inserts back at indexes 0 and 1); the count
 * is patched once, to int32(count + inserts), wrapping.
 * DG_EDIT_UNSET: each item is decided as a single UNSET; all items address the
 * ORIGINAL message (indexes do not shift between items); the count becomes
 * int32(count - dropped); a missed parent leaves the message unchanged, DG_EDIT_OK.
 * A message is edited as a whole or not at all: if an item's decision fails the
 * message fails with that item's status and aux (the first failing item in item
 * order) and nothing is written. Two items that resolve to overlapping spans
 * (STRKEY "a" and BINKEY "a" on one entry, an existing index given twice) are
 * DG_EDITM_E_SAME; the item reported is the second of the first overlapping pair
 * in message order (equal spans in item order). Two MISSING duplicates are a
 * legal double insert.
 * d_ret[i] = status | existed mask << 8 | failing item << 16 | aux << 32 (bit
 * 8 + j set when item j was a replace or a drop; the item field is 0 when OK); for
 * K = 1 the word is dg_edit's. d_out_len[i] as dg_edit's.
 *
 * Deviations from the reference besides 1-7:
 *   8. A replace checks the wire type (replaceMany does not).
 *   9. Overlapping items are DG_EDITM_E_SAME (replaceMany writes a corrupt buffer).
 *  10. Mixed step classes are refused by dg_editm_create with DG_E_ARG.
 *
 * dg_editm_create takes a DG_PATH_MAGIC blob of 1 to DG_EDITM_MAX_ITEMS paths of
 * equal length >= 1 that are identical in every step but the last: path j is
 * parent + item j's step. The blob is judged before the context is looked at
 * (DG_E_ARG with dg_path_create's texts, "N items", "paths of unequal length",
 * "paths differ before their last step", "mixed step classes"). Duplicate last
 * steps are not refused.
 */
typedef struct dg_editm dg_editm;
int dg_editm_create(dg_ctx *ctx, const void *path_blob, size_t len, uint32_t op, dg_editm **out);
void dg_editm_destroy(dg_editm *e);
uint32_t dg_editm_items(const dg_editm *e);
/* The exact worst case of one message's output: DG_EDIT_UNSET: len;
 * DG_EDIT_SET: len + val_total (the K values' lengths together) + the sum over
 * the items of what each last step can add (as dg_edit_slot_bound). */
uint64_t dg_editm_slot_bound(const dg_editm *e, uint64_t len, uint64_t val_total);
/* As dg_edit_batch_device (the arenas' spare bytes, the slot rules, max_len and
 * the routes "edit_lanes" / "edit_wave_min"); n * (K + 1) below 2^32. val_types
 * and val_lens are HOST arrays of K entries. With d_val_off (n * K + 1 entries,
 * message-major) item j of message i is d_val[d_val_off[i*K+j], d_val_off[i*K+j+1])
 * and val_lens[j] is the longest value of item j, a hint (0 = unknown); with
 * d_val_off NULL d_val holds the K values back to back (val_lens[j] bytes each)
 * and every message gets them. The lookup's (K + 1) n records live in the
 * scratch of the context that dg_edit_* uses too (it is this call with K = 1),
 * ordered across streams. */
int dg_editm_batch_device(dg_ctx *ctx, const dg_editm *e, uint8_t root_type, const uint8_t *d_thrift,
                          const uint64_t *d_in_off, uint64_t n, const uint8_t *val_types, const uint8_t *d_val,
                          const uint64_t *d_val_off, const uint64_t *val_lens, uint8_t *d_out,
                          const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret, void *stream,
                          uint64_t max_len);
/* Host buffers, synchronous, as dg_edit_batch_host: val_off has n * K + 1 entries
 * or is NULL (then val holds the K values back to back, val_lens[j] bytes each). */
int dg_editm_batch_host(dg_ctx *ctx, const dg_editm *e, uint8_t root_type, const uint8_t *thrift,
                        const uint64_t *in_off, uint64_t n, const uint8_t *val_types, const uint8_t *val,
                        const uint64_t *val_off, const uint64_t *val_lens, uint8_t *out, uint64_t out_cap,
                        uint64_t *out_off, uint64_t *ret, uint64_t *out_need);

/* ------------------------------------------------------------------------
 * kids: batched Children over Thrift-binary messages (the reference's
 * thrift/generic Node.Children / PathNode.scanChildren, node.go:1133-1154,
 * path.go:796-836, 1121-1248). For every message of a batch and the node at
 * the end of ONE path (a dg_path of exactly one path; the empty path is the
 * message's root) the table of the node's children, or with
 * DG_KIDS_F_RECURSE the whole subtree below it in preorder: what
 * v.GetByPath(path...) followed by .Children(&out, recurse, &Options{}) gives.
 *
 * The path is looked up as dg_tget_* does; a lookup that fails gives the
 * message its status (DG_TGET_NOT_FOUND / E_READ / E_TYPE) and step. A node
 * that is no struct, list, set or map is DG_KIDS_E_UNSUPPORTED
 * (meta.ErrUnsupportedType). The node's header, and in recursive mode every
 * nested container's, is read with ReadListBegin / ReadMapBegin (type bytes
 * Valid(), sizes not negative: stricter than the skip, so a list<type 5> of
 * size 0 is DG_TGET_E_READ here); every child's end comes from SkipType. Map
 * keys: a STRING key is DG_PS_STRKEY, an I08 / I16 / I32 / I64 key
 * DG_PS_INTKEY (ReadInt: an I08 key is unsigned), any other key type
 * DG_PS_BINKEY over the bytes SkipType delimits; keys are never descended
 * into. Any failure makes the message DG_TGET_E_READ with no records. Depth:
 * 1023 levels including the node for a non-empty path, 1023 below each direct
 * child for the empty path (the reference's outermost skip). Trailing bytes
 * after the root are ignored. The Go's storage options (StoreChildrenById,
 * StoreChildrenByHash, NotScanParentNode) have no counterpart: records come in
 * wire order and a container's record carries its real end.
 *
 * Records (dgj2t_defs.h): dg_kids_head per message, dg_kid_rec per child,
 * message i's at d_recs[d_rec_off[i], d_rec_off[i + 1]); d_rec_off[n] is the
 * total. head.direct of a list, set or map is Node.Len(), so a call without
 * d_recs is batched Len.
 *
 * Device buffers, stream-ordered, async (stream NULL: the context's). Messages
 * and root_type as dg_tget_batch_device (the arena readable 16 bytes past its
 * end; n below 2^32). d_head (n entries) and d_recs are 16-byte aligned,
 * d_rec_off has n + 1 entries. Stages: count kernel -> scan -> emit kernel.
 * d_recs NULL stops after the scan. DG_KIDS_F_COUNTED: d_head / d_rec_off were
 * filled by an earlier call with the same batch, path and flags; the call
 * emits only. A message whose records would pass rec_cap writes none and gets
 * DG_KIDS_E_OVERFLOW (count 0); no record is stored at an index >= rec_cap and
 * d_rec_off[n] still tells the need. A list, set or map node of fixed-size
 * entries with at least "kids_wide_min" children is emitted one lane per
 * record. n = 0 returns DG_OK and launches nothing. DG_E_ARG for a path set of
 * more or fewer than one path. max_len: the batch's longest message or 0, a
 * hint. */
int dg_kids_batch_device(dg_ctx *ctx, const dg_path *path, uint8_t root_type, uint32_t flags, const uint8_t *d_thrift,
                         const uint64_t *d_in_off, uint64_t n, dg_kids_head *d_head, uint64_t *d_rec_off,
                         dg_kid_rec *d_recs, uint64_t rec_cap, void *stream, uint64_t max_len);
/* Host buffers, synchronous (no spare bytes needed; DG_KIDS_F_COUNTED is
 * refused). head and rec_off are always filled and *need = rec_off[n]. recs
 * NULL with rec_cap 0 stops there (sizing, Len); otherwise DG_E_NOMEM when
 * rec_cap < *need, and no message is ever DG_KIDS_E_OVERFLOW. */
int dg_kids_batch_host(dg_ctx *ctx, const dg_path *path, uint8_t root_type, uint32_t flags, const uint8_t *thrift,
                       const uint64_t *in_off, uint64_t n, dg_kids_head *head, uint64_t *rec_off, dg_kid_rec *recs,
                       uint64_t rec_cap, uint64_t *need);

/* ------------------------------------------------------------------------
 * cols: typed column reads over Thrift-binary messages: GetByPath followed by
 * the reference's casts (thrift/generic/cast.go:50-224). A column is one path
 * plus a kind (dgj2t_defs.h DG_COL_*); cell (i, k) is what
 * v.GetByPath(path_k...) on message i and then the cast of column k's kind
 * give. A plan holds 1 to DG_TGET_MAX_PATHS columns; dg_cols_create takes
 * dg_path_create's blob with its limits and texts and n_kinds kinds, one per
 * path (DG_E_ARG with a text for an unknown kind or another count).
 *
 * A cell is a value (8 bytes), a dg_col_cell and, for STR and list columns, a
 * length:
 *   the lookup fails   status DG_TGET_NOT_FOUND / E_READ / E_TYPE with the
 *                      type, step and aux dg_tget_rec would hold; value 0.
 *   the cast does not take the wire type found
 *                      DG_COL_E_UNSUPPORTED (meta.ErrUnsupportedType), type =
 *                      the wire type found, step = the path length; value 0.
 *   DG_COL_BOOL        BOOL: 1 if the byte is exactly 1, else 0 (DecodeBool).
 *   DG_COL_BYTE        I08: the byte, 0..255.
 *   DG_COL_INT         I08 UNSIGNED (Node.Int goes through DecodeByte: 0x80 is
 *                      128); I16, I32, I64 big-endian, sign-extended.
 *   DG_COL_F64         DOUBLE: the 8 bytes byte-swapped, nothing else (NaN
 *                      payloads, -0.0 and denormals survive as bits).
 *   DG_COL_STR         STRING: value = the payload's offset in the arena
 *                      (d_in_off[i] + start + 4), length = end - start - 4:
 *                      the (offset, length) pair dg_pack_device_scan takes.
 *   DG_COL_LEN         LIST, SET: the i32 count at start + 1; MAP: at start + 2.
 *   DG_COL_LIST | DG_COL_INT, DG_COL_LIST | DG_COL_F64
 *                      for e in node.List(): e.Int() / e.Float64(). The node
 *                      must be LIST or SET (else E_UNSUPPORTED). Its header is
 *                      read as ReadListBegin reads it: an element type that
 *                      is not Valid() is DG_TGET_E_READ, step = the path
 *                      length, at any size. Size 0 with a valid element type:
 *                      OK, length 0. A non-empty list whose element type the
 *                      cast rejects (INT: anything but I08 / I16 / I32 / I64;
 *                      F64: anything but DOUBLE): E_UNSUPPORTED, type = the
 *                      node's, aux = the element type, no elements: a cell is
 *                      whole or empty. OK: length = the element count, value =
 *                      the arena offset of element 0, type = the element type.
 *                      Elements come out 8 bytes each: INT extended per width
 *                      (I08 unsigned), F64 bit for bit.
 * Elsewhere the length is 0. The reference's List() builds interface values
 * element by element and stops at the first that fails; here the element
 * type is checked once, in the header.
 */
typedef struct dg_cols dg_cols;
int dg_cols_create(dg_ctx *ctx, const void *path_blob, size_t len, const uint8_t *kinds, uint32_t n_kinds,
                   dg_cols **out);
void dg_cols_destroy(dg_cols *p);
uint32_t dg_cols_count(const dg_cols *p);

/* The cell pass. Device buffers, stream-ordered, async (stream NULL: the
 * context's); messages, root_type, the 16 readable bytes past the arena's end
 * and n * P < 2^32 as dg_tget_batch_device. Outputs are column-major, P = the
 * plan's column count: d_val (u64) and d_cell (dg_col_cell) hold P * n entries,
 * column k at [k * n, k * n + n), both 8-byte aligned; d_len (u32, P * n) may
 * be NULL when no column is STR or a list. n = 0 returns DG_OK and launches
 * nothing. Pairs nested beyond the 8 LDS skip frames are rerun by a deep pass
 * whose queue, counters and frames are the component's own. max_len: a hint. */
int dg_cols_batch_device(dg_ctx *ctx, const dg_cols *cols, uint8_t root_type, const uint8_t *d_thrift,
                         const uint64_t *d_in_off, uint64_t n, uint64_t *d_val, dg_col_cell *d_cell, uint32_t *d_len,
                         void *stream, uint64_t max_len);
/* The elements of list column k after dg_cols_batch_device on the same stream
 * (or ordered behind it): d_val_k / d_cell_k / d_len_k are column k's parts of
 * its outputs (d_val + k * n, ...). A scan of the counts fills d_elem_off (u64,
 * n + 1 entries, [n] = the total); then message i's elements go to
 * d_elems[d_elem_off[i], d_elem_off[i + 1]), 8 bytes each; empty and failed
 * cells contribute nothing. d_elems NULL stops after the scan (sizing). No
 * element is stored at an index >= elem_cap. DG_E_ARG when k names no list
 * column. */
int dg_cols_list_device(dg_ctx *ctx, const dg_cols *cols, uint32_t k, const uint8_t *d_thrift, uint64_t n,
                        const uint64_t *d_val_k, const dg_col_cell *d_cell_k, const uint32_t *d_len_k,
                        uint64_t *d_elem_off, uint64_t *d_elems, uint64_t elem_cap, void *stream);
/* Host buffers, synchronous (no spare bytes needed): val, cell and len (never
 * NULL here) as above, offsets relative to `thrift`. With L list columns,
 * elem_off has L * (n + 1) entries, the j-th list column's at [j * (n + 1), ...):
 * its message i owns elems[elem_off[i], elem_off[i + 1]), the columns' elements
 * one after the other, and *need = the last entry = all elements. elems NULL
 * with elem_cap 0 stops there (sizing); otherwise DG_E_NOMEM when elem_cap <
 * *need. elem_off may be NULL when L = 0. */
int dg_cols_batch_host(dg_ctx *ctx, const dg_cols *cols, uint8_t root_type, const uint8_t *thrift,
                       const uint64_t *in_off, uint64_t n, uint64_t *val, dg_col_cell *cell, uint32_t *len,
                       uint64_t *elem_off, uint64_t *elems, uint64_t elem_cap, uint64_t *need);

/* ------------------------------------------------------------------------
 * rows: row columns, the fields of every element of a list or set as ragged
 * columns: what the reference's loop
 *     v.GetByPath(parent...).Children(&kids, false, opts)
 *     for each kid: kid.Node.GetByPath(sub_k...) and the cast of column k
 * gives ("the price and the SKU of every line item of every order"). A plan is
 * ONE parent path (a path set of exactly one path; the empty path is the
 * message's root) plus 1 to DG_ROWS_MAX_COLS row columns, each a sub-path (it
 * may be empty) and a kind of cols (DG_COL_*). A component beside cols, ents
 * and kids: none of their entries changes.
 *
 *   head (message i)   the parent is looked up and its children scanned as
 *                      dg_kids_* does without DG_KIDS_F_RECURSE: a failed
 *                      lookup gives its status and step; under a non-empty
 *                      path the node is skipped first (a failure there is
 *                      DG_TGET_E_READ, step = the path's length) and its depth
 *                      budget starts one lower; a node that is not LIST or SET
 *                      is DG_COL_E_UNSUPPORTED with type = the wire type found
 *                      (a STRUCT or MAP parent too: dg_kids_* serves those);
 *                      the header is read as ReadListBegin reads it; an
 *                      element whose skip fails makes the message
 *                      DG_TGET_E_READ with no rows. OK: count = Node.Len().
 *   rows               d_row_off (u64, n + 1) is the exclusive scan of the
 *                      counts, d_row_off[n] the total R. Row d_row_off[i] + j
 *                      is element j of message i's list, in wire order; its
 *                      index entry (dg_row_ent) holds the element's arena
 *                      offset, its byte length and i.
 *   cell (g, k)        GetByPath(sub_k...) on the element's own bytes with the
 *                      list's element type as the root type and a fresh skip
 *                      budget, then column k's cast: a dg_cols_* cell, with
 *                      step counting within the sub-path. The lookup ends at
 *                      the element's end: a field that element j lacks and
 *                      element j + 1 has is DG_TGET_NOT_FOUND for row j. STR
 *                      and list cells hold arena offsets, as cols' do.
 * Children's storage options have no counterpart.
 */
typedef struct dg_rows dg_rows;
/* parent_blob: dg_path_create's blob of exactly one path; sub_blob: one of
 * n_kinds paths, kinds as dg_cols_create takes them (DG_E_ARG with a text
 * otherwise). */
int dg_rows_create(dg_ctx *ctx, const void *parent_blob, size_t parent_len, const void *sub_blob, size_t sub_len,
                   const uint8_t *kinds, uint32_t n_kinds, dg_rows **out);
void dg_rows_destroy(dg_rows *p);
uint32_t dg_rows_count(const dg_rows *p);

/* Device buffers, stream-ordered, async (stream NULL: the context's), all
 * passes on the one stream with no host round trip: head/count pass -> scan ->
 * index pass -> row cell pass, each lane pass followed by its deep pass.
 * Messages, root_type and the 16 readable bytes past the arena's end as
 * dg_tget_batch_device; n below 2^32. d_head (n entries) and d_index are
 * 16-byte aligned, d_row_off has n + 1 entries. Outputs are column-major over
 * row_cap, P = the plan's column count: d_val (u64), d_cell (dg_col_cell) and
 * d_len (u32, NULL allowed when no column is STR or a list) hold P * row_cap
 * entries, column k at [k * row_cap, ...), the first two 8-byte aligned.
 * d_index (row_cap entries) may be NULL: the index then lives in the
 * component's own scratch. Rows [0, min(R, row_cap)) are indexed and their
 * cells written; no index entry and no cell of a row >= row_cap is ever stored
 * and d_row_off[n] still tells the need. d_val and d_cell NULL is the sizing
 * call: heads and d_row_off only (with d_index given, the index as well: the
 * first two passes and the third). row_cap * P must stay below 2^32
 * (DG_E_INVALID with a text). n = 0 writes d_row_off[0] = 0 and launches
 * nothing else. The deep passes' queue, counters and frames and the scan's
 * tile sums are the component's own. max_len: a hint. */
int dg_rows_batch_device(dg_ctx *ctx, const dg_rows *rows, uint8_t root_type, const uint8_t *d_thrift,
                         const uint64_t *d_in_off, uint64_t n, dg_rows_head *d_head, uint64_t *d_row_off,
                         dg_row_ent *d_index, uint64_t *d_val, dg_col_cell *d_cell, uint32_t *d_len, uint64_t row_cap,
                         void *stream, uint64_t max_len);
/* The elements of list-kind row column k after dg_rows_batch_device on the
 * same stream (or ordered behind it), as dg_cols_list_device over rows: n_rows
 * = the rows whose cells were written (min(R, row_cap)), d_val_k / d_cell_k /
 * d_len_k column k's parts of its outputs (d_val + k * row_cap, ...). A scan
 * fills d_elem_off (u64, n_rows + 1 entries); row g's elements go to
 * d_elems[d_elem_off[g], d_elem_off[g + 1]), 8 bytes each. d_elems NULL stops
 * after the scan; no element is stored at an index >= elem_cap. DG_E_ARG when k
 * names no list column. */
int dg_rows_list_device(dg_ctx *ctx, const dg_rows *rows, uint32_t k, const uint8_t *d_thrift, uint64_t n_rows,
                        const uint64_t *d_val_k, const dg_col_cell *d_cell_k, const uint32_t *d_len_k,
                        uint64_t *d_elem_off, uint64_t *d_elems, uint64_t elem_cap, void *stream);
/* Host buffers, synchronous (no spare bytes needed): head (n) and row_off
 * (n + 1) are always filled and *need = row_off[n] = R. index, val, cell and
 * len all NULL with row_cap 0 stops there (sizing); otherwise DG_E_NOMEM when
 * row_cap < *need and DG_E_INVALID when R * P reaches 2^32. val, cell and len
 * (never NULL then) are column-major over row_cap, rows [0, R) of each column
 * written; index (R entries) may be NULL. Offsets are relative to `thrift`. */
int dg_rows_batch_host(dg_ctx *ctx, const dg_rows *rows, uint8_t root_type, const uint8_t *thrift,
                       const uint64_t *in_off, uint64_t n, dg_rows_head *head, uint64_t *row_off, dg_row_ent *index,
                       uint64_t *val, dg_col_cell *cell, uint32_t *len, uint64_t row_cap, uint64_t *need);

/* Map plans: the entries of a map<K, V> as rows, with their keys ("the price of
 * every SKU in prices: map<string, Item>"): what the reference's loop
 *     v.GetByPath(parent...).Children(&kids, false, opts)
 *     for each kid: kid.Path is the key; kid.Node.GetByPath(sub_k...) and the
 *                   cast of column k is the cell
 * gives over a MAP node. A map plan is a rows plan with a key kind
 * (DG_ROWS_KEY_STR or DG_ROWS_KEY_INT); a list plan behaves as above, and a
 * MAP parent under a list plan stays DG_COL_E_UNSUPPORTED.
 *
 *   head (message i)   in this order: the lookup's status and step on failure
 *                      (under a non-empty path the node's skip comes first,
 *                      DG_TGET_E_READ with step = the path's length on failure,
 *                      and the depth budget starts one lower); a node that is
 *                      not MAP (LIST and SET too) is DG_COL_E_UNSUPPORTED with
 *                      type = the wire type found; the header is read as
 *                      ReadMapBegin reads it (a key or value type that is not
 *                      Valid(), or a negative size, is DG_TGET_E_READ); a key
 *                      type the plan's key kind does not take (STR: STRING
 *                      only; INT: I08 / I16 / I32 / I64 only) is
 *                      DG_COL_E_UNSUPPORTED with type = MAP and elem_type = the
 *                      key type found, at any size, 0 included; an entry whose
 *                      key or value fails to skip makes the message
 *                      DG_TGET_E_READ with no rows. OK: count = Node.Len(),
 *                      type = MAP, elem_type = the VALUE type (the root type of
 *                      every row's lookup), first = the arena offset of entry
 *                      0's key, the byte after the 6-byte header.
 *                      The key-type rule deviates: the reference's Children
 *                      yields PathBinKey for other key types; the restriction
 *                      is StrMap's / IntMap's, as in dg_ents_*.
 *   rows               in wire order, duplicate keys kept. The index entry
 *                      (dg_row_ent) is the VALUE's span and the message.
 *   key (row g)        d_key[g]: an int key is the value as ReadInt and
 *                      dg_kid_rec.key give it (I08 unsigned: 0xFF is 255; I16,
 *                      I32, I64 sign-extended); a string key is the arena
 *                      offset of its payload. d_key_len[g]: a string key's
 *                      payload length; an int key's width in bytes (1, 2, 4 or
 *                      8), which tells the wire type. No key of a row >=
 *                      row_cap is stored.
 *   cell (g, k)        exactly the list plan's, on the value's own bytes; the
 *                      lookup's end is the value's end.
 */
/* As dg_rows_create with its limits and texts (one parent path, 1 to
 * DG_ROWS_MAX_COLS sub-paths, cols' kinds); an unknown key_kind is DG_E_ARG
 * with a text. */
int dg_rows_create_map(dg_ctx *ctx, const void *parent_blob, size_t parent_len, const void *sub_blob, size_t sub_len,
                       const uint8_t *kinds, uint32_t n_kinds, uint32_t key_kind, dg_rows **out);
/* DG_ROWS_KEY_STR or DG_ROWS_KEY_INT; 0 for a list plan (and for NULL) */
uint32_t dg_rows_key_kind(const dg_rows *p);
/* dg_rows_batch_device / dg_rows_batch_host for a map plan: their arguments,
 * sizing call, index-only call, row_cap rules, row_cap * P < 2^32 rule and
 * n = 0, plus d_key (u64, row_cap entries, 8-byte aligned) and d_key_len (u32,
 * row_cap entries), each of which may be NULL: not wanted. The keys are
 * written by the index pass, for exactly the rows whose index entries are
 * (into d_index or the component's scratch). The host entry's string-key
 * offsets are relative to `thrift`. A list plan here, and a map plan at
 * dg_rows_batch_device / dg_rows_batch_host, is DG_E_ARG with a text;
 * dg_rows_list_device takes both, since it only reads cells. */
int dg_rows_map_batch_device(dg_ctx *ctx, const dg_rows *rows, uint8_t root_type, const uint8_t *d_thrift,
                             const uint64_t *d_in_off, uint64_t n, dg_rows_head *d_head, uint64_t *d_row_off,
                             dg_row_ent *d_index, uint64_t *d_key, uint32_t *d_key_len, uint64_t *d_val,
                             dg_col_cell *d_cell, uint32_t *d_len, uint64_t row_cap, void *stream, uint64_t max_len);
int dg_rows_map_batch_host(dg_ctx *ctx, const dg_rows *rows, uint8_t root_type, const uint8_t *thrift,
                           const uint64_t *in_off, uint64_t n, dg_rows_head *head, uint64_t *row_off, dg_row_ent *index,
                           uint64_t *key, uint32_t *key_len, uint64_t *val, dg_col_cell *cell, uint32_t *len,
                           uint64_t row_cap, uint64_t *need);

/* ------------------------------------------------------------------------
 * ents: entry columns, the containers cols leaves out: GetByPath followed by
 * Node.List with String per element, Node.StrMap or Node.IntMap
 * (thrift/generic/cast.go:198-286), for a whole batch, as ragged columns. A
 * column is one path plus a kind (dgj2t_defs.h DG_ENT_*); a plan holds 1 to
 * DG_TGET_MAX_PATHS columns; dg_ents_create takes dg_path_create's blob with
 * its limits and texts and n_kinds kinds, one per path (DG_E_ARG with a text
 * for an unknown kind or another count). A component beside cols: dg_cols_*
 * takes none of these kinds.
 *
 * A cell is a value (8 bytes), a dg_col_cell, a length and a span:
 *   the lookup fails   status DG_TGET_NOT_FOUND / E_READ / E_TYPE with the
 *                      type, step and aux dg_tget_rec would hold; value 0.
 *   the node is of another container class (LISTSTR: not LIST or SET; the map
 *   kinds: not MAP)    DG_COL_E_UNSUPPORTED, type = the wire type found,
 *                      step = the path length, aux 0.
 *   DG_ENT_LISTSTR     the header as ReadListBegin reads it: an element type
 *                      that is not Valid() is DG_TGET_E_READ (type 0, step =
 *                      the path length) at any size. Size 0 with a valid
 *                      element type: OK, length 0. Size > 0 and an element
 *                      type other than STRING: E_UNSUPPORTED, aux = the
 *                      element type. OK: type = the element type, value = the
 *                      arena offset of element 0 (its length prefix).
 *   DG_ENT_STRMAP | v  ReadMapBegin first: a key or value type that is not
 *                      Valid() is DG_TGET_E_READ (type 0, aux 0) at any size.
 *                      Then a key type other than STRING is E_UNSUPPORTED at
 *                      any size, size 0 included.
 *   DG_ENT_INTMAP | v  the key byte is tested BEFORE the header is read: a key
 *                      byte that is not I08 / I16 / I32 / I64, valid or not, is
 *                      E_UNSUPPORTED with aux = that byte alone (the value
 *                      byte was not read). Then a value type that is not
 *                      Valid() is DG_TGET_E_READ (type 0, aux 0).
 *   both map kinds     every cell whose header was read carries it in aux:
 *                      key type | value type << 8. Size 0: OK, length 0,
 *                      whatever the value type. Size > 0 and a value type the
 *                      value kind rejects (INT: anything but I08 / I16 / I32 /
 *                      I64; F64: but DOUBLE; BOOL: but BOOL; STR: but STRING):
 *                      E_UNSUPPORTED. OK: type = MAP, value = the arena offset
 *                      of the first entry (its key).
 * An OK cell's length is the count and its span the bytes from the value's
 * offset to the container's end, which the lookup's final skip found: the
 * emit's walk never reads an entry past it. Elsewhere value, length and span
 * are 0. A body cut short or a negative count never reaches the cast: the
 * lookup's skip has made it DG_TGET_E_READ. Entries come out in wire order
 * with duplicate keys kept (a Go map keeps the last and has no order), and
 * the value type is checked once, on the header.
 */
typedef struct dg_ents dg_ents;
int dg_ents_create(dg_ctx *ctx, const void *path_blob, size_t len, const uint8_t *kinds, uint32_t n_kinds,
                   dg_ents **out);
void dg_ents_destroy(dg_ents *p);
uint32_t dg_ents_count(const dg_ents *p);

/* The cell pass: dg_cols_batch_device's contract (device buffers, stream-
 * ordered, async, column-major outputs of P * n entries, the 16 readable bytes
 * past the arena, n * P < 2^32, n = 0 launches nothing) with d_len required
 * and d_span (u32, P * n) beside it. The deep pass's queue, counters and
 * frames are the component's own. */
int dg_ents_batch_device(dg_ctx *ctx, const dg_ents *ents, uint8_t root_type, const uint8_t *d_thrift,
                         const uint64_t *d_in_off, uint64_t n, uint64_t *d_val, dg_col_cell *d_cell, uint32_t *d_len,
                         uint32_t *d_span, void *stream, uint64_t max_len);
/* Column k's entries after dg_ents_batch_device on the same stream (or ordered
 * behind it): d_val_k / d_cell_k / d_len_k / d_span_k are column k's parts of
 * its outputs (d_val + k * n, ...). A scan of the counts fills d_ent_off (u64,
 * n + 1 entries, [n] = the total); message i owns the slots [d_ent_off[i],
 * d_ent_off[i + 1]) of up to four arrays:
 *   d_key (u64)      an int key as ReadInt reads it (I08 unsigned: 0xFF is
 *                    255; I16 / I32 / I64 sign-extended); a string key: the
 *                    arena offset of its payload. Not written by LISTSTR.
 *   d_key_len (u32)  string keys: the payload's length. Written by the STRMAP
 *                    kinds alone.
 *   d_val (u64)      the value as the cols cell of its kind decodes it (BOOL:
 *                    1 if the byte is exactly 1; INT: I08 unsigned, the rest
 *                    sign-extended; F64: bit for bit); a string value or a
 *                    LISTSTR element: the arena offset of its payload.
 *   d_val_len (u32)  string values and elements: the payload's length.
 *                    Written by LISTSTR and the STR value kinds alone.
 * The (offset, length) pairs are the ones dg_pack_device_scan takes. An array
 * the caller does not need may be NULL; all four NULL stops after the scan
 * (sizing). No slot at an index >= ent_cap is stored; empty and failed cells
 * contribute nothing. DG_E_ARG when k names no column. */
int dg_ents_emit_device(dg_ctx *ctx, const dg_ents *ents, uint32_t k, const uint8_t *d_thrift, uint64_t n,
                        const uint64_t *d_val_k, const dg_col_cell *d_cell_k, const uint32_t *d_len_k,
                        const uint32_t *d_span_k, uint64_t *d_ent_off, uint64_t *d_key, uint32_t *d_key_len,
                        uint64_t *d_val, uint32_t *d_val_len, uint64_t ent_cap, void *stream);
/* Host buffers, synchronous (no spare bytes needed): val, cell and len (P * n
 * each, never NULL when n > 0) as above, offsets relative to `thrift`. ent_off
 * has P * (n + 1) entries, column k's at [k * (n + 1), ...): its message i owns
 * the slots [ent_off[i], ent_off[i + 1]) of key / key_len / ent_val /
 * ent_val_len, the columns' entries one after the other, and *need = the last
 * entry = all entries. The four arrays NULL with ent_cap 0 stops there
 * (sizing); otherwise DG_E_NOMEM when ent_cap < *need, and an array that is
 * NULL is not filled. Slots of an array a column's kind does not write hold 0. */
int dg_ents_batch_host(dg_ctx *ctx, const dg_ents *ents, uint8_t root_type, const uint8_t *thrift,
                       const uint64_t *in_off, uint64_t n, uint64_t *val, dg_col_cell *cell, uint32_t *len,
                       uint64_t *ent_off, uint64_t *key, uint32_t *key_len, uint64_t *ent_val, uint32_t *ent_val_len,
                       uint64_t ent_cap, uint64_t *need);

/* ------------------------------------------------------------------------
 * vals: typed column writes, the inverse of cols: tensors encoded to
 * Thrift-binary values (the reference's NewNodeBool ... NewNodeString /
 * NewNodeBinary / NewNodeList / NewNodeSet, thrift/generic/node.go:92-201, over
 * WriteAny, thrift/binary.go:1480-1682, and BinaryEncoding.Encode*,
 * binary.go:2101-2149) or, with field ids, to whole struct messages
 * (NewNodeStruct). A plan holds K columns, 1 <= K <= DG_VALS_MAX_COLS, each
 * with a kind (dgj2t_defs.h DG_VAL_*); a batch has n * K < 2^32 cells.
 * dg_vals_create answers DG_E_ARG with a text naming the kind and the column
 * for any other kind, and for another K.
 *
 * What cell (i, k) writes, from column k's dg_val_col at row i:
 *   BOOL               one byte, 1 if the 64-bit input is non-zero, else 0
 *                      (EncodeBool).
 *   I08 I16 I32 I64    the low 8 / 16 / 32 / 64 bits of the input, big-endian:
 *                      Go's int16(x) conversion. Nothing is range-checked and
 *                      nothing is an error, so what DG_COL_INT read from a
 *                      field of a width and what is written at that width are
 *                      the same bytes (an I08 read as 0..255 writes its low
 *                      byte).
 *   DOUBLE             the 8 input bytes swapped and nothing else (NaN
 *                      payloads, the signalling bit, -0.0 and denormals
 *                      survive as bits, as DG_COL_F64 reads them).
 *   STRING             the i32 big-endian length d_len[i], then the d_len[i]
 *                      bytes at d_src + d_val[i] (EncodeString / EncodeBinary).
 *   LIST / SET         the element type byte, the i32 big-endian count
 *                      d_elem_off[i + 1] - d_elem_off[i], then the elements
 *                      d_elems[d_elem_off[i] ...] encoded as the scalars above.
 *                      Count 0 is legal: the kind names the element type
 *                      (WriteAny refuses an empty []interface{}).
 * Lists of strings, structs or containers, maps, and descriptor-aware writes
 * (WriteAnyWithDesc) are not part of this: lists and sets of strings and maps
 * are dg_evals_* below, the rest stays out.
 *
 * Cell errors: a STRING length or a list count above 2^31 - 1, or an item
 * (the value and, in struct mode, its field header and STOP) of 2^32 bytes or
 * more, is DG_VAL_E_SIZE: the cell is flagged in d_status and written as the
 * empty value of its kind (00 00 00 00; elem 00 00 00 00), so the arena always
 * holds well-formed Thrift. Every other cell is DG_VAL_OK.
 *
 * Struct mode (field_ids given, K of them): item j of a message is preceded by
 * EncodeFieldBegin(wire type, field_ids[j]), 3 bytes, and the last item of
 * every message is followed by the STOP byte, so message i is
 * d_out[d_out_off[i * K], d_out_off[(i + 1) * K]). Fields go in column order
 * (Go's map order is unspecified). d_present[i] == 0 leaves column k's field
 * out of message i; a message with no field present is the STOP byte alone.
 * Without field ids a d_present pointer is DG_E_ARG at the call.
 */
typedef struct dg_vals dg_vals;
int dg_vals_create(dg_ctx *ctx, const uint8_t *kinds, uint32_t K, const int16_t *field_ids, dg_vals **out);
void dg_vals_destroy(dg_vals *p);
uint32_t dg_vals_count(const dg_vals *p);
/* the wire type of column k's values (dg_editm_batch_device's val_types[k]):
 * the kind itself for a scalar, 15 for a list, 14 for a set; 0 for no such column */
uint8_t dg_vals_wire_type(const dg_vals *p, uint32_t k);

/* Device buffers, stream-ordered, async (stream NULL: the context's). cols: K
 * records in HOST memory whose pointers are device pointers. The outputs are
 * a message-major arena, dg_editm_batch_device's d_val / d_val_off: d_out_off
 * (u64, n * K + 1 entries, 8-byte aligned), [i * K + j] the start of item j of
 * message i, [0] = out_base, the last entry the arena's end; d_out the bytes,
 * cap + 16 allocated, nothing stored at an index >= cap and the 16 spare bytes
 * untouched; d_status (u8, n * K, message-major) may be NULL. d_out NULL stops
 * after the offsets and statuses (sizing). n = 0 returns DG_OK and launches
 * nothing. Three steps: a size pass (a plan of scalars only, with no d_present,
 * has closed-form offsets: no scan, and the same launch writes the bytes), the
 * scan of the lengths (cols' scan; the lengths and the tile sums are the
 * component's own, one set per context, ordered across streams like every
 * shared workspace), and the emit: a head pass, one lane per cell, and a body
 * pass in which whole waves store string payloads and list elements in
 * contiguous runs. Knob "vals_lane_emit" = 1: one lane per cell writes all of
 * it (the baseline the measurements compare with). */
int dg_vals_batch_device(dg_ctx *ctx, const dg_vals *plan, const dg_val_col *cols, uint64_t n, uint64_t out_base,
                         uint8_t *d_out, uint64_t cap, uint64_t *d_out_off, uint8_t *d_status, void *stream);
/* Host buffers, synchronous (no spare bytes needed): cols' pointers are host
 * pointers, out_off (n * K + 1, never NULL) starts at 0, status may be NULL.
 * *need = the arena's bytes. out NULL with cap 0 stops there (sizing);
 * otherwise DG_E_NOMEM when cap < *need. */
int dg_vals_batch_host(dg_ctx *ctx, const dg_vals *plan, const dg_val_col *cols, uint64_t n, uint8_t *out, uint64_t cap,
                       uint64_t *out_off, uint8_t *status, uint64_t *need);

/* ------------------------------------------------------------------------
 * evals: entry column writes, the inverse of ents and a component beside vals
 * (dg_vals_* takes none of these kinds): ragged tensors encoded to list<string>,
 * set<string> and map values (the reference's NewNodeList / NewNodeSet /
 * NewNodeMap, thrift/generic/node.go:154-187, over WriteAny,
 * thrift/binary.go:1480-1660) or, with field ids, to struct messages of such
 * fields. A plan holds K columns, 1 <= K <= DG_VALS_MAX_COLS, each with a
 * uint16_t kind (dgj2t_defs.h): DG_VAL_LIST | 11, DG_VAL_SET | 11, or
 * DG_EVAL_MAP | kt << 4 | vt with kt one of 3, 6, 8, 10, 11 and vt one of 2, 3,
 * 4, 6, 8, 10, 11. dg_evals_create answers DG_E_ARG ("column j: unknown kind
 * N") for any other kind, and for another K.
 *
 * What cell (i, k) writes, from column k's dg_eval_col: message i owns the
 * entries [d_ent_off[i], d_ent_off[i + 1]) of the per-entry arrays, in the
 * shapes dg_ents_emit_device writes them (its outputs plug in unchanged, with
 * d_thrift as both arenas).
 *   list / set   0B, the i32 big-endian count, then every element: its i32
 *                length d_val_len[e] and the bytes at d_val_src + d_val[e].
 *   map          kt, vt, the i32 count, then every entry as its key followed
 *                by its value. A scalar is encoded as dg_vals encodes it (BOOL:
 *                1 for any non-zero input; integers: the low bits big-endian;
 *                DOUBLE: the eight bytes swapped), a string as its i32 length
 *                and payload.
 * Struct mode (field_ids given) is dg_vals': the 3-byte field header before
 * every item, STOP behind a message's last, d_present[i] == 0 leaves the field
 * out, and a d_present pointer without field ids is DG_E_ARG at the call.
 *
 * Deviations from the reference:
 *   1. Count 0 is legal: the kind names the types (WriteAny refuses an empty
 *      container).
 *   2. Entries are written in input order and a key given twice is written
 *      twice (a Go map has no order and no duplicates).
 *   3. Struct and container values, map[interface{}], WriteAnyWithDesc and keys
 *      of other types stay out.
 *   4. A plan holds entry kinds only: a message of scalar and entry columns
 *      takes two calls, dg_vals in struct mode and then dg_editm (set_many) to
 *      insert the containers.
 *
 * Cell errors; a flagged cell is written as the empty container of its kind
 * (0B 00 00 00 00; kt vt 00 00 00 00), so the arena always holds well-formed
 * Thrift, and none of its entries' payload bytes is read:
 *   DG_VAL_E_SIZE     a count above 2^31 - 1, any key or value length of the
 *                     cell above 2^31 - 1, or an item of 2^32 bytes or more.
 *   DG_EVAL_E_RANGE   d_ent_off[i] > d_ent_off[i + 1], or d_ent_off[i + 1] >
 *                     n_ent. RANGE is tested first.
 * No entry at an index >= n_ent is ever read. Entry ranges may overlap or leave
 * gaps: every cell reads its own range.
 */
typedef struct dg_evals dg_evals;
int dg_evals_create(dg_ctx *ctx, const uint16_t *kinds, uint32_t K, const int16_t *field_ids, dg_evals **out);
void dg_evals_destroy(dg_evals *p);
uint32_t dg_evals_count(const dg_evals *p);
/* the wire type of column k's values (dg_editm_batch_device's val_types[k]):
 * 15 for a list, 14 for a set, 13 for a map; 0 for no such column */
uint8_t dg_evals_wire_type(const dg_evals *p, uint32_t k);
/* the bytes of d_work a batch of n messages needs whose column k holds
 * n_ent[k] entries (K values): the cells' lengths, counts and scanned counts,
 * per variable-stride column 12 bytes an entry (its encoded size and its
 * position), and the scans' tile sums. 0 for a NULL argument, n >= 2^32 or an
 * n_ent above DG_EVALS_MAX_ENT. */
uint64_t dg_evals_work_bytes(const dg_evals *p, uint64_t n, const uint64_t *n_ent);

/* Device buffers, stream-ordered, async (stream NULL: the context's). cols: K
 * records in HOST memory whose pointers are device pointers. The outputs are
 * dg_vals_batch_device's message-major arena: d_out_off (u64, n * K + 1
 * entries, 8-byte aligned), [0] = out_base, the last entry the arena's end;
 * d_out with cap + 16 bytes allocated, nothing stored at an index >= cap and
 * the 16 spare bytes untouched; d_status (u8, n * K) may be NULL. d_out NULL
 * stops after the offsets and statuses (sizing). n = 0 returns DG_OK and
 * launches nothing. d_work (8-byte aligned, work_bytes >=
 * dg_evals_work_bytes, else DG_E_NOMEM) is the call's only storage: nothing is
 * allocated, and calls on several streams need a d_work each. An n_ent above
 * DG_EVALS_MAX_ENT is DG_E_ARG. Per variable-stride column (a string key, a
 * string value, list elements) an entry-size pass, one lane per entry, and
 * cols' scan; then for all columns at once a cell pass, the scans of the
 * cells' lengths (into d_out_off) and counts, a head pass and ONE
 * entry-parallel emit over the entries of every column, in which a lane writes
 * one entry's key and value whatever the containers' sizes are. */
int dg_evals_batch_device(dg_ctx *ctx, const dg_evals *plan, const dg_eval_col *cols, uint64_t n, uint64_t out_base,
                          uint8_t *d_out, uint64_t cap, uint64_t *d_out_off, uint8_t *d_status, void *d_work,
                          uint64_t work_bytes, void *stream);
/* Host buffers, synchronous (no spare bytes needed, no d_work): cols' pointers
 * are host pointers, out_off (n * K + 1, never NULL) starts at 0, status may be
 * NULL. *need = the arena's bytes. out NULL with cap 0 stops there (sizing);
 * otherwise DG_E_NOMEM when cap < *need. */
int dg_evals_batch_host(dg_ctx *ctx, const dg_evals *plan, const dg_eval_col *cols, uint64_t n, uint8_t *out, uint64_t cap,
                        uint64_t *out_off, uint8_t *status, uint64_t *need);

/* ------------------------------------------------------------------------
 * rvals: row column writes, the inverse of rows and a component beside vals
 * and evals (neither takes struct elements): ragged row tensors encoded to
 * list<struct> and set<struct> values (the reference's NewNodeList /
 * NewNodeSet over []interface{} of map[FieldID]interface{},
 * thrift/generic/node.go:154-187, over WriteAny, thrift/binary.go:1504-1528 and
 * :1661). A plan holds the outer container's wire type, 15 (LIST) or 14 (SET),
 * and K columns, 1 <= K <= DG_VALS_MAX_COLS, each with one of vals' 19 kinds
 * (the six fixed-width scalars, STRING, DG_VAL_LIST | elem and DG_VAL_SET | elem
 * over the six) and a field id; the field ids are required, the elements being
 * structs. Lists of bare scalars stay with dg_vals_*, lists of strings with
 * dg_evals_*. dg_rvals_create answers DG_E_ARG with a text naming it for any
 * other kind ("column j: unknown kind N"), K, container or for no field ids.
 *
 * Inputs: d_row_off (u64, n + 1), the array dg_rows_batch_device writes:
 * message i owns the rows [d_row_off[i], d_row_off[i + 1]) of the per-row
 * arrays, which hold n_rows rows (a host value, as evals' n_ent). cols: K
 * dg_val_col records indexed by row: d_val[n_rows], d_len[n_rows], d_src,
 * d_elem_off[n_rows + 1], d_elems, d_present[n_rows] (optional), the shapes
 * dg_rows_batch_device and dg_rows_list_device write, so their outputs plug in
 * unchanged. n_rows * K < 2^32 (the scan's limit) and n < 2^32.
 *
 * What message i writes: one item, in the form dg_editm_batch_device takes as
 * d_val / d_val_off for one item of wire type 15 or 14: 0C, the i32 big-endian
 * count, then its rows in order. A row is every present column in column
 * order, each as EncodeFieldBegin(wire type, id), 3 bytes, and the value as
 * dg_vals writes it in struct mode, then 00 (STOP). A row with no column
 * present is the STOP byte alone; an empty list is 5 bytes.
 *
 * Statuses, both arrays optional:
 *   d_status (u8, n)  DG_EVAL_E_RANGE: d_row_off[i] > d_row_off[i + 1] or
 *                     d_row_off[i + 1] > n_rows, tested first. DG_VAL_E_SIZE: a
 *                     count above 2^31 - 1, or an item of 2^32 bytes or more.
 *                     Either writes the message as the empty container
 *                     (0C 00 00 00 00).
 *   d_cell_status (u8, n_rows * K, row-major)  vals' DG_VAL_E_SIZE rule per
 *                     cell, unchanged: the flagged cell is written as the empty
 *                     value of its kind, the row and the message stay OK.
 * The per-row arrays (values, lengths, element offsets, present) are read for
 * every row below n_rows and for none at or beyond it. No payload byte and no
 * element is read for a row that no OK message owns, for an absent cell or for
 * a flagged cell. Row ranges may overlap or leave gaps, as evals' entry ranges:
 * a row owned by two messages is written twice.
 *
 * Deviations from the reference:
 *   1. Count 0 is legal (WriteAny refuses an empty []interface{}).
 *   2. Fields go in column order (Go's map order is unspecified).
 *   3. Nested structs, maps, strings inside inner lists and WriteAnyWithDesc
 *      stay out.
 *   4. The struct message around the list stays out: the item is inserted with
 *      dg_editm (set_many), as evals' deviation 4 does.
 */
typedef struct dg_rvals dg_rvals;
int dg_rvals_create(dg_ctx *ctx, const uint8_t *kinds, uint32_t K, const int16_t *field_ids, uint8_t container,
                    dg_rvals **out);
void dg_rvals_destroy(dg_rvals *p);
uint32_t dg_rvals_count(const dg_rvals *p);
/* the wire type of every message's item (dg_editm_batch_device's val_types[k]): 15 or 14; 0 for a NULL plan */
uint8_t dg_rvals_wire_type(const dg_rvals *p);
/* the bytes of d_work that suffice for any batch of n messages over n_rows
 * rows: per cell its length and its position (12 bytes), per message its
 * length, its count and its scanned count (16 bytes), and one set of tile sums.
 * A plan of scalars whose columns all come without d_present (the fixed-stride
 * route) uses the per-message part and the sums only, and the call takes a
 * d_work of that size. 0 for a NULL plan, n >= 2^32 or n_rows * K >= 2^32. */
uint64_t dg_rvals_work_bytes(const dg_rvals *p, uint64_t n, uint64_t n_rows);

/* Device buffers, stream-ordered, async (stream NULL: the context's). cols: K
 * records in HOST memory whose pointers are device pointers. The output is a
 * message-major arena with one item per message: d_out_off (u64, n + 1 entries,
 * 8-byte aligned), [0] = out_base, [n] the arena's end; d_out with cap + 16
 * bytes allocated, nothing stored at an index >= cap and the 16 spare bytes
 * untouched. d_out NULL stops after the offsets and statuses (sizing). n = 0
 * returns DG_OK and launches nothing. d_work (8-byte aligned; short: DG_E_NOMEM)
 * is the call's only storage: nothing is allocated, and calls on several
 * streams need a d_work each. The passes: a cell-size pass, one lane per (row,
 * column), and cols' scan of the lengths (neither on the fixed-stride route); a
 * message pass, one lane per message, and the scans of the messages' lengths
 * (into d_out_off) and row counts; a head pass, one lane per cell of every
 * emitted row; and, for a plan with a STRING or container column, vals' body
 * pass over the arena's bytes, in which whole waves store contiguous runs. Rows
 * are placed by the scans and written row-parallel, so one message of 10 000
 * rows costs what the same rows cost spread evenly. */
int dg_rvals_batch_device(dg_ctx *ctx, const dg_rvals *plan, const dg_val_col *cols, const uint64_t *d_row_off, uint64_t n,
                          uint64_t n_rows, uint64_t out_base, uint8_t *d_out, uint64_t cap, uint64_t *d_out_off,
                          uint8_t *d_status, uint8_t *d_cell_status, void *d_work, uint64_t work_bytes, void *stream);
/* Host buffers, synchronous (no spare bytes needed, no d_work): cols' pointers
 * and row_off are host pointers, out_off (n + 1, never NULL) starts at 0,
 * status (n) and cell_status (n_rows * K) may be NULL. The per-row arrays are
 * uploaded whole, payloads and elements from the first to the last byte a live
 * cell reads. *need = the arena's bytes. out NULL with cap 0 stops there
 * (sizing); otherwise DG_E_NOMEM when cap < *need. */
int dg_rvals_batch_host(dg_ctx *ctx, const dg_rvals *plan, const dg_val_col *cols, const uint64_t *row_off, uint64_t n,
                        uint64_t n_rows, uint8_t *out, uint64_t cap, uint64_t *out_off, uint8_t *status, uint8_t *cell_status,
                        uint64_t *need);

/* Timing helper for benchmarks: launch the device batch `iters` times on the
 * context stream bracketed by HIP events; returns total milliseconds of GPU
 * time in *ms (events are recorded on the stream the kernels run on). */
int dg_bench_device(dg_ctx *ctx, const dg_desc *desc, uint32_t root_type, const uint8_t *d_json,
                    const uint64_t *d_in_off, uint64_t n, uint64_t flags, uint8_t *d_out,
                    const uint64_t *d_out_off, uint32_t *d_out_len, uint64_t *d_ret, int iters,
                    float *ms);

#ifdef __cplusplus
}
#endif
#endif /* DGJ2T_H */
