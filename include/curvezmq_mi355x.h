/*
 * curvezmq_mi355x.h -- C-ABI of the MI355X CurveZMQ MESSAGE crypto path.
 *
 * This library replaces, for JeroMQ's CURVE sockets, the per-message NaCl calls
 * that JeroMQ makes through the third-party jnacl artefact
 * (eu.neilalexander:jnacl:1.0.0, jeromq-core/pom.xml:18-22; imported at
 * jeromq-core/src/main/java/zmq/io/mechanism/curve/Curve.java:5-6).
 * Every entry point is plain C: pointers, sizes, ints.  Device pointers are
 * HIP device addresses; `stream` is a hipStream_t passed as void* (NULL = the
 * null stream).  All batched launchers are asynchronous, allocate nothing and
 * never synchronise, so they may be captured into a hipGraph.
 *
 * Return conventions
 *   jnacl drop-ins (section 1): 0 on success, -1 on failure -- exactly the
 *   int contract of crypto_box_afternm / crypto_box_open_afternm that
 *   Curve.java:134-147 forwards to callers (encode asserts rc == 0,
 *   CurveClientMechanism.java:153-154; decode maps -1 to EPROTO,
 *   CurveClientMechanism.java:218-223).
 *   Everything else: CZ_OK (0) or a negative CZ_E* code; cz_last_error()
 *   returns a thread-local message.
 *
 * Thread safety: all functions are reentrant.  The single-shot calls use a
 * per-thread device context (JeroMQ runs one connection per IO thread,
 * StreamEngine.java:467-535); cz_ctx objects must not be shared between
 * threads without external locking.
 */
#ifndef CURVEZMQ_MI355X_H
#define CURVEZMQ_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Sizes: Curve.Size (Curve.java:14-67) / jnacl crypto_secretbox_* constants */
#define CZ_NONCEBYTES 24
#define CZ_ZEROBYTES 32
#define CZ_BOXZEROBYTES 16
#define CZ_KEYBYTES 32
#define CZ_BEFORENMBYTES 32
#define CZ_MACBYTES 16
/* MESSAGE body = "\x07MESSAGE"(8) + nonce8 + tag16 + flags(1) + payload */
#define CZ_MESSAGE_OVERHEAD 33
/* largest MESSAGE payload: the body (payload + 33) must fit a Java int, as every Msg size does
 * (Msg.java size(): int); encode / encode_batch / cz_engine_send return CZ_EMSGSIZE beyond it */
#define CZ_MESSAGE_MAX (0x7fffffff - CZ_MESSAGE_OVERHEAD)

/* Msg flags carried in the encrypted flags byte (Msg.java:96-100, CurveClientMechanism.java:131-137) */
#define CZ_MSG_MORE 0x01
#define CZ_MSG_COMMAND 0x02

/* direction of a connection-direction subkey (nonce prefix, CurveClientMechanism.java:141, :182) */
#define CZ_DIR_C2S 0 /* "CurveZMQMESSAGEC": sealed by the client, opened by the server */
#define CZ_DIR_S2C 1 /* "CurveZMQMESSAGES": sealed by the server, opened by the client */

/* Per-frame status of an open (low byte) -- what Mechanism.decode would have raised */
#define CZ_STATUS_OK 0
#define CZ_STATUS_CRYPTO 1    /* bad tag: ZMQ_PROTOCOL_ERROR_ZMTP_CRYPTOGRAPHIC (zmq/ZMQ.java:227) */
#define CZ_STATUS_MALFORMED 2 /* size < 33: ZMTP_MALFORMED_COMMAND_MESSAGE (CurveClientMechanism.java:174-178) */
#define CZ_STATUS_COMMAND 3   /* not "\x07MESSAGE": ZMTP_UNEXPECTED_COMMAND (CurveClientMechanism.java:168-172) */
#define CZ_STATUS_SEQUENCE 4  /* nonce <= previous: replay (CurveClientMechanism.java:186-193) */
/* bits 8..15 of an OK status hold the decrypted flags byte (CZ_MSG_MORE / CZ_MSG_COMMAND) */

/* Library error codes */
#define CZ_OK 0
#define CZ_EINVAL (-22)
#define CZ_EHIP (-5)
#define CZ_ENOMEM (-12)
#define CZ_EPROTO (-71)
#define CZ_EMSGSIZE (-90)
#define CZ_EAGAIN (-11)

/* cz_frame_desc.flags bits (seal: low byte = the MESSAGE flags byte) */
#define CZ_DESC_CHECK_NONCE 0x100 /* open: enforce nonce > floor (counter or prev frame's nonce) */

/*
 * One frame of a batch (40 bytes).  Offsets are byte offsets into the batch's
 * in / out buffers, any alignment.  The segment kernels store outputs at any byte offset
 * through line staging (whole 128-byte cache lines) and read payloads / bodies at any byte
 * offset with dword-aligned loads (16-byte aligned inputs are fastest).
 *   seal: in  = payload (len = n bytes)      out = MESSAGE body (n + 33 bytes)
 *         counter = the 8-byte nonce counter (cnNonce), flags low byte = MORE|COMMAND
 *   open: in  = MESSAGE body (len = size)    out = payload (size - 33 bytes)
 *         counter = replay floor (cnPeerNonce) used when prev < 0;
 *         prev >= 0: the floor is the nonce of frame `prev` of this batch (same connection)
 *   key_idx selects the 32-byte Salsa20 subkey in the batch's subkey table.
 */
typedef struct cz_frame_desc {
    uint64_t in_off;
    uint64_t out_off;
    uint32_t len;
    uint32_t key_idx;
    uint64_t counter;
    uint32_t flags;
    int32_t prev;
} cz_frame_desc;

/* ---- 1. jnacl drop-ins (host memory, NaCl ZEROBYTES layouts) -------------------
 * Replaces curve25519xsalsa20poly1305.crypto_box_afternm (called at Curve.java:136)
 * and crypto_box_open_afternm (Curve.java:146); crypto_secretbox[_open]
 * (xsalsa20poly1305, Curve.java:166,176) is the same primitive.
 * NaCl's crypto_secretbox for every m, as jnacl and libsodium: c = keystream ^ m over all mlen
 * bytes, the Poly1305 key is c[0:32] = keystream[0:32] ^ m[0:32] (so an m whose first 32 bytes
 * are not zero -- Curve.box, Curve.java:184-193, accepts any m -- gets NaCl's tag, not an error),
 * the tag lands at c[16:32] and c[0:16] is written as zero.  The open keys the MAC with the
 * keystream (crypto_secretbox_open), returns -1 on a bad tag with m untouched, and writes
 * m[0:32] as zero.  Runs on the GPU in one launch per call (every seal whose m[0:32] is not zero,
 * and boxes up to 80 KiB; larger CurveZMQ boxes through the segmented kernels): latency-bound,
 * ~11 us of launch + sync floor -- use the batched API for throughput. */
int cz_box_afternm(uint8_t *c, const uint8_t *m, uint64_t mlen, const uint8_t n[24], const uint8_t k[32]);
int cz_box_open_afternm(uint8_t *m, const uint8_t *c, uint64_t clen, const uint8_t n[24], const uint8_t k[32]);
/* The one-launch drop-ins above keep, per calling thread, the HSalsa20 subkeys of the last 8
 * (k, n[0:16]) pairs in device memory (CurveZMQ: one pair per connection direction), so repeated
 * calls on a connection skip the derivation.  Wipe this thread's cache (host copy of the keys and
 * the device subkeys). */
int cz_nacl_forget(void);
/* Create the calling thread's single-shot contexts (the drop-ins' HIP stream, device buffers and
 * pinned staging, and the handshake calls') now instead of on its first call.  Optional; the JNI
 * shim calls it once per thread before it pins any Java array, so HIP runtime initialisation never
 * runs while the JVM's GC is locked out (GetPrimitiveArrayCritical).  CZ_OK or CZ_EHIP. */
int cz_nacl_thread_init(void);
int cz_secretbox(uint8_t *c, const uint8_t *m, uint64_t mlen, const uint8_t n[24], const uint8_t k[32]);
int cz_secretbox_open(uint8_t *m, const uint8_t *c, uint64_t clen, const uint8_t n[24], const uint8_t k[32]);

/* ---- 2. key schedule ------------------------------------------------------------
 * Per-connection-direction Salsa20 subkey = HSalsa20(cnPrecom, "CurveZMQMESSAGE{C|S}").
 * The MESSAGE nonce is that constant 16-byte prefix + BE64(counter)
 * (CurveClientMechanism.java:139-142), so XSalsa20's HSalsa20 step is hoisted
 * out of the per-message path.  d_precom / d_subkeys: nkeys x 32 bytes (device). */
int cz_subkeys(void *d_subkeys, const void *d_precom, uint32_t nkeys, int direction, void *stream);
/* host convenience: one subkey (runs the same device kernel, synchronously) */
int cz_subkey(uint8_t out[32], const uint8_t k[32], int direction);

/* ---- 3. batched, device-resident -----------------------------------------------
 * Mechanism.encode / decode for `count` independent frames in one launch.
 * d_order (optional, count x u32) permutes the lane->frame assignment: pass the
 * frames sorted by decreasing length to balance ragged batches (cz_plan_order). */
int cz_seal_batch(const cz_frame_desc *d_desc, const uint32_t *d_order, uint32_t count, const void *d_in,
                  void *d_out, const void *d_subkeys, void *stream);
/* d_status[i] = CZ_STATUS_* | (flags << 8); d_nonces (optional) = the frame's nonce counter */
int cz_open_batch(const cz_frame_desc *d_desc, const uint32_t *d_order, uint32_t count, const void *d_in,
                  void *d_out, const void *d_subkeys, uint16_t *d_status, uint64_t *d_nonces, void *stream);

/* Uniform-length batch of ONE connection direction: frame i at in + i*in_stride,
 * body i at out + i*out_stride, nonce counter0 + i, flags d_flags8[i] (NULL = 0).
 * Any strides and base alignments: payloads packed at any byte offset are read with
 * dword-aligned loads.
 * OUTPUT OWNERSHIP, decided by out_stride alone (the same rule as section 3c): with an
 * out_stride that is a multiple of 128 below 32 MiB (2^25), or a multiple of 16 of at most
 * 256 (64 slots in 16 KiB), the batch owns count * out_stride output bytes and every slot
 * byte past a body is written as zero, whatever the length, the count and the base
 * alignments (full waves of 16-byte aligned slots store whole 128-byte lines once; other
 * layouts and the last partial wave store lane by lane and zero the rest of the slot
 * themselves).  With any other out_stride -- e.g. bodies back to back, 4129 bytes apart
 * at 4 KiB, or slots of 32 MiB and more -- only the count bodies are written and the bytes
 * between them stay as the caller wrote them (below 4 MiB through byte-shifted line
 * staging, lane by lane above). */
int cz_seal_uniform(uint32_t count, uint32_t len, const void *d_in, uint64_t in_stride, void *d_out,
                    uint64_t out_stride, const void *d_subkey, uint64_t counter0, const uint8_t *d_flags8,
                    void *stream);
/* The same batch from input already in the reference's NaCl box layout: slot i holds the box
 * m = 0^32 || flags || payload (len = payload bytes, so a box is len + 33 bytes), exactly the
 * buffer CurveClientMechanism.encode builds and hands to Curve.afternm (CurveClientMechanism.java:
 * 144-153, Curve.java:134-137).  The flags byte comes from box byte 32; box bytes 0..31 are not
 * read.  Output as cz_seal_uniform.  Input read where it lies: no byte shift on the device. */
int cz_seal_uniform_box(uint32_t count, uint32_t len, const void *d_box, uint64_t box_stride, void *d_out,
                        uint64_t out_stride, const void *d_subkey, uint64_t counter0, void *stream);
/* Open `count` bodies of `size` bytes of one connection in order; frame 0 must
 * beat floor0, frame i must beat frame i-1 (when check != 0).  Payload i goes to
 * out + i*out_stride.  Bodies at any byte offset (in_stride 4129: the dense wire
 * layout) are read with dword-aligned loads.  Output ownership by out_stride alone, the
 * rule of cz_seal_uniform: a multiple of 128 below 32 MiB, or a multiple of 16 of at most
 * 256 -- the batch owns count * out_stride output bytes (slot bytes past a payload, and
 * rejected frames' whole slots, are written as zero); any other out_stride -- bytes
 * between payloads untouched, rejected frames' payload bytes written as zero. */
int cz_open_uniform(uint32_t count, uint32_t size, const void *d_in, uint64_t in_stride, void *d_out,
                    uint64_t out_stride, const void *d_subkey, uint64_t floor0, int check, uint16_t *d_status,
                    void *stream);

/* Host-side planner: order[] = frame indices sorted by decreasing len (stable). */
int cz_plan_order(const cz_frame_desc *h_desc, uint32_t count, uint32_t *h_order);

/* ---- 3b. segmented (ragged) batches ---------------------------------------------
 * One lane per frame makes a long frame the batch's critical path (a 64 KiB frame is
 * 1025 sequential Salsa20 blocks on one lane).  cz_plan_segments splits frames longer
 * than 1.5 x seg_blocks 64-byte blocks into seg_blocks-block segments (the last one
 * takes the remainder; for open, segments s >= 1 start at block s*seg_blocks + 1),
 * sorts segments longest first (by output chunks), and lists the split frames for
 * the combine step, which joins the per-segment Poly1305 partials with r^m powers.
 * d_work must hold 64 bytes per part (*npart from the planner).  Output contract as
 * cz_seal_batch / cz_open_batch (statuses, nonces, zeroed plaintext on a bad tag).
 * A caller may also build its own plan: the segments of a split frame cover its box blocks
 * [0, nblk) contiguously, one or more blocks each (open: segments after the first start at
 * block 2 or later), with consecutive part indices from the frame's part0, in any order in
 * the list and of any lengths (tests/test_gpu_segments.py cuts frames at random points). */
typedef struct cz_segment {
    uint32_t frame;       /* index into the descriptor array */
    uint32_t first_block; /* first 64-byte box block of the segment */
    uint32_t nblocks;
    uint32_t part;        /* partial-record index, 0xffffffff for a frame in one segment */
} cz_segment;
typedef struct cz_combine {
    uint32_t frame;
    uint32_t part0; /* first partial record of the frame (its segments are consecutive) */
    uint32_t nseg;
    uint32_t reserved;
} cz_combine;
/* open = 0: desc.len is a payload length (seal); 1: a body size (open).  Returns CZ_EINVAL
 * with *nseg / *ncomb set to the sizes needed when a capacity is too small. */
int cz_plan_segments(const cz_frame_desc *h_desc, uint32_t count, int open, uint32_t seg_blocks, cz_segment *h_seg,
                     uint32_t seg_cap, uint32_t *nseg, cz_combine *h_comb, uint32_t comb_cap, uint32_t *ncomb,
                     uint32_t *npart);
int cz_seal_segments(const cz_frame_desc *d_desc, const cz_segment *d_seg, uint32_t nseg, const cz_combine *d_comb,
                     uint32_t ncomb, const void *d_in, void *d_out, const void *d_subkeys, void *d_work,
                     void *stream);
int cz_open_segments(const cz_frame_desc *d_desc, const cz_segment *d_seg, uint32_t nseg, const cz_combine *d_comb,
                     uint32_t ncomb, const void *d_in, void *d_out, const void *d_subkeys, void *d_work,
                     uint16_t *d_status, uint64_t *d_nonces, void *stream);

/* ---- 3c. fan-out: one payload sealed for many connections ------------------------
 * A PUB / XPUB socket hands the SAME Msg to every matching pipe (Dist.distribute,
 * zmq/socket/pubsub/Dist.java -> write(pipe, msg)), and each pipe's StreamEngine runs
 * mechanism.encode on it under its own key and nonce: N seals of one payload.  Here that is one
 * launch, one lane per subscriber, with a 16-byte record per subscriber instead of a 40-byte
 * descriptor and a 16-byte segment per frame.  Body i = the MESSAGE body of d_payload[0, len)
 * with flags byte `flags` (as cz_frame_desc.flags) under subkey d_subs[i].key_idx and nonce
 * d_subs[i].counter, at d_out + i*out_stride: exactly the bytes cz_seal_batch writes for count
 * descriptors that share one in_off.
 * Output ownership as cz_seal_uniform: with an out_stride that is a multiple of 128 (below
 * 32 MiB), or a multiple of 16 with 64 slots in 16 KiB (out_stride <= 256), the batch owns
 * count * out_stride bytes and slot bytes past a body are written as zero; with any other
 * out_stride >= len + 33 the bytes between bodies are left as the caller wrote them.  Full waves
 * of 16-byte aligned slots store whole lines; partial waves, other strides, and an output base
 * or payload off 16-byte alignment store lane by lane (correct, not tuned).
 * count == 0: CZ_OK, nothing launched.  Null pointers, out_stride < len + 33: CZ_EINVAL;
 * len > CZ_MESSAGE_MAX: CZ_EMSGSIZE (checked before the device is touched).  No device: CZ_EHIP. */
typedef struct cz_fanout_sub {
    uint64_t counter;  /* nonce counter of this subscriber's frame */
    uint32_t key_idx;  /* subkey index */
    uint32_t reserved; /* 0 */
} cz_fanout_sub;
/* Dist.distribute (zmq/socket/pubsub/Dist.java) -> write(pipe, msg) -> mechanism.encode per pipe */
int cz_seal_fanout(uint32_t count, uint32_t len, const void *d_payload, uint32_t flags,
                   const cz_fanout_sub *d_subs, const void *d_subkeys,
                   void *d_out, uint64_t out_stride, void *stream);

/* ---- 3d. grouped fan-out: many publishes sealed in one call -------------------------
 * A publisher under load hands Dist.distribute one Msg after another, each to its own list of
 * pipes; one cz_seal_fanout launch per Msg runs them one after the other, each far too small for
 * the device.  Here R runs -- each the cz_seal_fanout of one payload for `count` subscribers -- are
 * one call of at most three launches whatever R: one lane per (run, subscriber), every run padded
 * to whole 64-lane waves, a per-wave record naming the run a wave serves.  Planner and launch as
 * cz_plan_segments + cz_seal_segments.
 * Run r seals d_in[payload_off, payload_off + len) with flags byte `flags` for subscribers
 * d_subs[first_sub .. first_sub + count), body j at d_out + out_off + j*out_stride: byte for byte
 * what cz_seal_fanout(count, len, d_in + payload_off, flags, d_subs + first_sub, d_subkeys,
 * d_out + out_off, out_stride) writes, ownership rule of section 3c per run included.
 * CALLER'S CONTRACT: the output ranges of different runs (count * out_stride bytes for a run that
 * owns its slots, (count - 1) * out_stride + len + 33 otherwise) must not overlap; runs may share
 * payloads and subscriber records.
 * The staging class of a wave (line emitter, region emitter, lane-wise) is the one cz_seal_fanout
 * picks for its run alone, from the run's stride and length and the 16-byte alignment of
 * d_in + payload_off and d_out + out_off; partial waves are lane-wise.  The planner sorts waves by
 * class, longest payload first inside a class.  The class only decides which launch a wave rides
 * in: the kernel re-checks the run's alignment and strides itself and stores lane-wise when they
 * do not fit, so a table planned for other base addresses is slower, never wrong. */
typedef struct cz_fanout_run {
    uint64_t payload_off; /* payload's byte offset in d_in */
    uint64_t out_off;     /* first body slot's byte offset in d_out */
    uint64_t out_stride;  /* >= len + 33 */
    uint32_t len;         /* payload bytes, <= CZ_MESSAGE_MAX */
    uint32_t flags;       /* as cz_frame_desc.flags (low byte) */
    uint32_t first_sub;   /* index of the run's first cz_fanout_sub */
    uint32_t count;       /* subscribers; 0 = the run contributes nothing */
} cz_fanout_run;           /* 40 bytes */
typedef struct cz_fanout_wave {
    uint32_t run;   /* index into the run array */
    uint32_t first; /* the wave's lane 0 serves this subscriber of the run (a multiple of 64) */
} cz_fanout_wave;
/* order of the classes in the wave table and in class_count[] */
#define CZ_FANOUT_LINES 0
#define CZ_FANOUT_REGION 1
#define CZ_FANOUT_DIRECT 2
/* Host-side planner, no device call; d_in and d_out are used as addresses only (alignment class).
 * Every run is validated before anything is written: len > CZ_MESSAGE_MAX -> CZ_EMSGSIZE;
 * out_stride < len + 33, first_sub + count past 2^32, out_off + count * out_stride past the
 * address space, null pointers -> CZ_EINVAL.  *nwaves = sum of ceil(count / 64); a wave_cap below
 * that (or a null h_waves) returns CZ_EINVAL with *nwaves set and nothing else written, as
 * cz_plan_segments.  class_count[c] = waves of class c (they sum to *nwaves); *region_stride =
 * the largest out_stride among the region-class runs (0: none), which sizes that launch's LDS.
 * Replaces the per-Msg loop of Dist.distribute (zmq/socket/pubsub/Dist.java) -> write(pipe, msg)
 * -> mechanism.encode, once per message and per pipe. */
int cz_plan_fanout(const cz_fanout_run *h_runs, uint32_t nruns, const void *d_in, const void *d_out,
                   cz_fanout_wave *h_waves, uint32_t wave_cap, uint32_t *nwaves, uint32_t class_count[3],
                   uint32_t *region_stride);
/* Dist.distribute (zmq/socket/pubsub/Dist.java) -> write(pipe, msg) -> mechanism.encode, once per
 * message and per pipe: all of it for R messages.  d_runs / d_waves: device copies of the run array
 * and of the planner's wave table; class_count and region_stride as the planner returned them
 * (region_stride 0 = the largest region slot, 256).  nruns == 0 or no waves: CZ_OK, nothing
 * launched.  Null pointers: CZ_EINVAL (checked before the device is touched).  No device: CZ_EHIP;
 * there is no CPU fallback. */
int cz_seal_fanout_runs(const cz_fanout_run *d_runs, uint32_t nruns, const cz_fanout_wave *d_waves,
                        const uint32_t class_count[3], uint32_t region_stride, const void *d_in,
                        const cz_fanout_sub *d_subs, const void *d_subkeys, void *d_out, void *stream);

/* ---- 3e. split fan-out: long publishes on a subscriber x segment grid ------------------
 * Sections 3c and 3d keep a frame on one lane, so a publish takes the time one lane needs for its
 * blocks whatever the number of subscribers.  Here the lanes are (run, subscriber, segment): a wave
 * holds 64 subscribers of one run on one segment of the body, so payload, length, flags and block
 * range are wave-uniform and the plan is one 24-byte record per WAVE -- no descriptor per frame, no
 * segment record per (frame, segment).  The runs are the cz_fanout_run array of section 3d, unchanged.
 * Cut points as cz_plan_segments makes them for one seal descriptor of the run's length: a body of
 * nblk = ceil((len + 33) / 64) blocks stays whole when nblk <= seg_blocks + seg_blocks / 2, and is
 * ceil(nblk / seg_blocks) segments of seg_blocks blocks otherwise, the last one the remainder.  The
 * tiles of a split run leave 64-byte Poly1305 partial records in d_work (record part + lane * nseg
 * for the tile's lane, so a subscriber's nseg records are consecutive), and one join lane per
 * (split run, subscriber) combines them into the tag at body byte 16.
 * OUTPUT: for every run, byte for byte what cz_seal_fanout writes for that run alone, ownership
 * rule of section 3c included; the caller keeps the runs' output ranges disjoint, as in 3d.
 * A tile's class (CZ_FANOUT_TILE_LINES: a full wave of a 16-byte aligned payload, line-staged
 * stores; CZ_FANOUT_TILE_DIRECT: partial waves and other payloads, lane-wise) only decides which
 * launch the wave rides in: a wave re-checks its own run and stores lane-wise when it does not fit
 * the line emitters, so a table planned for other addresses is slower, never wrong.
 * A caller may build its own tables: the tiles of one (run, 64 subscribers) cover the body's blocks
 * [0, nblk) contiguously, one or more blocks each, any lengths, in any order in the table, with
 * part = the wave's first record + the segment's index and the same nseg in each. */
typedef struct cz_fanout_tile {
    uint32_t run;         /* index into the run array */
    uint32_t first;       /* the wave's lane 0 serves this subscriber of the run (a multiple of 64) */
    uint32_t first_block; /* first 64-byte box block of the tile */
    uint32_t nblocks;     /* clipped to the body's block count by the kernel */
    uint32_t part;        /* lane 0's partial record, 0xffffffff for a body in one tile */
    uint32_t nseg;        /* segments of the body: lane l writes record part + l * nseg */
} cz_fanout_tile;          /* 24 bytes */
typedef struct cz_fanout_join {
    uint32_t run;   /* index into the run array (a split run) */
    uint32_t first; /* the wave's lane 0 serves this subscriber of the run (a multiple of 64) */
    uint32_t part;  /* lane 0's first partial record; lane l combines [part + l * nseg, + nseg) */
    uint32_t nseg;
} cz_fanout_join;    /* 16 bytes */
/* order of the classes in the tile table and in class_count[] */
#define CZ_FANOUT_TILE_LINES 0
#define CZ_FANOUT_TILE_DIRECT 1
/* Host-side planner, no device call; d_in is used as an address only (alignment class).
 * seg_blocks == 0: the segment length cz_engine_flush_out picks for a batch of the call's total
 * blocks whose longest body is the longest run's.  Every refusal of cz_plan_fanout applies, checked
 * before anything is written; more than 2^32 - 1 tiles, join waves or partial records: CZ_EINVAL.
 * *ntiles = sum over runs of segments x ceil(count / 64), *njoins = sum over split runs of
 * ceil(count / 64), *npart = sum over split runs of count x segments (d_work must hold 64 bytes
 * each).  A tile_cap / join_cap below that (or a null table) returns CZ_EINVAL with the three
 * sizes set and nothing else written, as cz_plan_segments.  class_count[c] = tiles of class c;
 * inside a class the tiles with the most blocks come first.
 * Replaces the per-Msg loop of Dist.distribute (zmq/socket/pubsub/Dist.java) -> write(pipe, msg)
 * -> mechanism.encode, once per message and per pipe. */
int cz_plan_fanout_split(const cz_fanout_run *h_runs, uint32_t nruns, const void *d_in, uint32_t seg_blocks,
                         cz_fanout_tile *h_tiles, uint32_t tile_cap, uint32_t *ntiles, uint32_t class_count[2],
                         cz_fanout_join *h_joins, uint32_t join_cap, uint32_t *njoins, uint32_t *npart);
/* Dist.distribute (zmq/socket/pubsub/Dist.java) -> write(pipe, msg) -> mechanism.encode, once per
 * message and per pipe: all of it for R messages, in at most three launches whatever R (tiles of
 * the line class, lane-wise tiles, join).  d_runs / d_tiles / d_joins: device copies of the run
 * array and of the planner's tables; class_count as the planner returned it.  Asynchronous on
 * `stream`; allocates nothing.  nruns == 0 or no tiles: CZ_OK, nothing launched.  Null pointers
 * (d_joins / d_work only when njoins != 0): CZ_EINVAL, checked before the device is touched.  No
 * device: CZ_EHIP; there is no CPU fallback. */
int cz_seal_fanout_split(const cz_fanout_run *d_runs, uint32_t nruns, const cz_fanout_tile *d_tiles,
                         const uint32_t class_count[2], const cz_fanout_join *d_joins, uint32_t njoins,
                         const void *d_in, const cz_fanout_sub *d_subs, const void *d_subkeys, void *d_out,
                         void *d_work, void *stream);

/* ---- 3f. fan-in: same-size bodies of many connections opened in one call -----------------
 * The mirror image of sections 3c and 3d: a collector in front of thousands of publishers, a ROUTER
 * taking small requests, a SUB with many upstreams.  Every connection's StreamEngine runs
 * mechanism.decode on each of its frames under its own key and cnPeerNonce (StreamEngine.decodeAndPush
 * -> mechanism.decode, once per message and per connection: StreamEngine.java:1067-1098,
 * CurveClientMechanism.java:166-224, CurveServerMechanism.java:165-225).  Here R runs of same-size
 * bodies are one call of at most three launches whatever R: one lane per body, a 16-byte record per
 * body instead of a 40-byte descriptor and a 16-byte segment, a per-wave record naming the run.
 * Body j of a run lies at d_in + in_off + j * in_stride (`size` bytes), its payload goes to
 * d_out + out_off + j * out_stride, and its record, status and nonce are d_subs / d_status / d_nonces
 * [first_sub + j] (d_nonces optional).  Payload bytes, status (CZ_STATUS_* | flags << 8) and nonce
 * are what cz_open_batch produces for the descriptor {in, out, size, key_idx, counter = the floor,
 * CZ_DESC_CHECK_NONCE or not, prev = -1}; a bad tag zeroes the plaintext, and a frame rejected before
 * decryption gets zeros over its payload bytes.
 * CZ_FANIN_FLOOR_IS_BODY: `floor` is a byte offset into d_in, and the floor is the wire nonce (BE64
 * at +8) of the body that starts there, accepted or not -- the connection's previous body, in this
 * run, in another, or in no run at all.  That is what lets a chain cross run edges and reach bodies
 * that stay in a segment plan, with a 16-byte record and no index space for `prev`.
 * Output ownership per run by out_stride alone, the rule of cz_open_uniform: an owning stride gets
 * zeros past each payload and over rejected frames' whole slots; any other stride leaves the bytes
 * between payloads untouched.  The kernel writes its own zeros (no zero-pad launch).  The caller
 * keeps the runs' output ranges and record ranges disjoint.  size < 33: every frame is COMMAND or
 * MALFORMED and nothing but owned slots' zeros is written.
 * A full wave's class is the staging cz_open_uniform's rule gives the run's out_stride and payload
 * length when d_in + in_off, in_stride, d_out + out_off and out_stride are all 16-byte aligned
 * (lane-wise otherwise); partial waves are lane-wise.  Waves are sorted by class, longest size first.
 * The class only decides which launch a wave rides in: a wave re-checks its own run's alignment,
 * stride limits and LDS partition and stores lane-wise when they do not fit, so a table planned for
 * other addresses is slower, never wrong. */
#define CZ_FANIN_CHECK_NONCE 0x1   /* enforce nonce > floor (signed, as CZ_DESC_CHECK_NONCE) */
#define CZ_FANIN_FLOOR_IS_BODY 0x2 /* `floor` is a byte offset into d_in: the floor is the wire nonce
                                      (BE64 at +8) of the body that starts there -- the connection's
                                      previous body, in this run, in another, or in no run at all */
typedef struct cz_fanin_sub {  /* 16 bytes, one per body */
    uint64_t floor;    /* cnPeerNonce, or a body offset with CZ_FANIN_FLOOR_IS_BODY */
    uint32_t key_idx;  /* subkey index */
    uint32_t flags;    /* CZ_FANIN_* */
} cz_fanin_sub;
typedef struct cz_fanin_run {  /* 48 bytes */
    uint64_t in_off, in_stride;   /* body j at d_in + in_off + j * in_stride, `size` bytes */
    uint64_t out_off, out_stride; /* payload j at d_out + out_off + j * out_stride */
    uint32_t size;                /* body bytes of every frame of the run */
    uint32_t first_sub;           /* record, status and nonce index of body 0 */
    uint32_t count;               /* 0 = the run contributes nothing */
    uint32_t reserved;
} cz_fanin_run;
/* Host-side planner, no device call; d_in and d_out are used as addresses only (alignment class).
 * Every run is validated before anything is written: size above 0x7fffffff, with count > 1 an
 * out_stride below the payload length or an in_stride below size, first_sub + count past 2^32, an
 * offset sum past the address space, null pointers -> CZ_EINVAL.  *nwaves = sum of ceil(count / 64); a
 * wave_cap below that (or a null h_waves) returns CZ_EINVAL with *nwaves set and nothing else written,
 * as cz_plan_fanout.  class_count[c] = waves of class c (CZ_FANOUT_LINES / _REGION / _DIRECT);
 * *region_stride as cz_plan_fanout.
 * Replaces StreamEngine.decodeAndPush -> mechanism.decode, once per message and per connection
 * (StreamEngine.java:1067-1098, CurveClientMechanism.java:166-224, CurveServerMechanism.java:165-225). */
int cz_plan_fanin(const cz_fanin_run *h_runs, uint32_t nruns, const void *d_in, const void *d_out,
                  cz_fanout_wave *h_waves, uint32_t wave_cap, uint32_t *nwaves, uint32_t class_count[3],
                  uint32_t *region_stride);
/* StreamEngine.decodeAndPush -> mechanism.decode, once per message and per connection
 * (StreamEngine.java:1067-1098, CurveClientMechanism.java:166-224, CurveServerMechanism.java:165-225):
 * all of it for R runs, in at most three launches whatever R.  d_runs / d_waves: device copies of the
 * run array and of the planner's wave table; class_count and region_stride as the planner returned
 * them.  Asynchronous on `stream`; allocates nothing; can be captured into a graph.  nruns == 0 or no
 * waves: CZ_OK, nothing launched.  Null pointers (d_nonces is optional): CZ_EINVAL, checked before the
 * device is touched.  No device: CZ_EHIP; there is no CPU fallback. */
int cz_open_fanin_runs(const cz_fanin_run *d_runs, uint32_t nruns, const cz_fanout_wave *d_waves,
                       const uint32_t class_count[3], uint32_t region_stride, const void *d_in,
                       const cz_fanin_sub *d_subs, const void *d_subkeys, void *d_out,
                       uint16_t *d_status, uint64_t *d_nonces, void *stream);

/* ---- 3g. split fan-in: long received bodies on a connection x segment grid ----------------
 * Section 3f keeps a body on one lane, so a run takes the time one lane needs for its blocks whatever the
 * number of connections.  Here the lanes are (run, body, segment), the mirror image of section 3e: a wave
 * holds 64 bodies of one run on one segment, so size, strides, bases and block range are wave-uniform
 * and the plan is one 24-byte cz_fanout_tile per WAVE -- no descriptor per frame, no segment record per
 * (frame, segment).  Runs and per-body records are the cz_fanin_run / cz_fanin_sub arrays of section 3f,
 * unchanged (CZ_FANIN_CHECK_NONCE, CZ_FANIN_FLOOR_IS_BODY); tiles, joins and classes are the
 * cz_fanout_tile / cz_fanout_join / CZ_FANOUT_TILE_* of section 3e, with `first` the wave's first body.
 * Cut points as cz_plan_segments makes them for one open descriptor of the run's size: a body of
 * nblk = ceil(size / 64) blocks stays whole when nblk <= seg_blocks + seg_blocks / 2, and is
 * ceil((nblk - 1) / seg_blocks) segments otherwise -- segment 0 covers blocks [0, seg_blocks + 1), segment
 * s >= 1 starts at block s * seg_blocks + 1, the last one takes the remainder.  seg_blocks == 1 is legal
 * here: a body of one or two blocks stays whole, a longer one is blocks [0, 2) and then one block per
 * segment.  The tiles of a split run leave 64-byte Poly1305 partial records in d_work (record
 * part + lane * nseg for the tile's lane, `part` including the segment's index, so a body's nseg records
 * are consecutive), and one join lane per (split run, body) combines them, compares with the tag at body
 * byte 16 and writes the status.
 * OUTPUT: for every run, byte for byte what cz_open_fanin_runs writes for the same runs and records --
 * payload bytes, d_status[first_sub + j] (CZ_STATUS_* | flags << 8), d_nonces[first_sub + j] (optional),
 * zeros over the payload bytes of a frame rejected before decryption and over the plaintext of a frame
 * whose tag fails, and the ownership rule of cz_open_uniform per run by out_stride alone (an owning
 * stride gets zeros past each payload and over rejected frames' whole slots; any other stride leaves the
 * bytes between payloads untouched).  The kernels write their own zeros (no zero-pad launch); nothing
 * outside the runs' output and record ranges is touched.  The caller keeps the runs' output ranges and
 * record ranges disjoint, as in section 3f.
 * A tile's class (CZ_FANOUT_TILE_LINES: a full wave whose body base d_in + in_off and in_stride are
 * 16-byte aligned, line-staged stores; CZ_FANOUT_TILE_DIRECT: every other tile, lane-wise) only decides
 * which launch the wave rides in: a wave re-checks its own run, and opens lane-wise when it does not
 * fit the line emitters or holds a frame rejected before decryption, so a table planned for other
 * addresses is slower, never wrong.
 * A caller may build its own tables under the rule of section 3b for open: the tiles of one (run, 64
 * bodies) cover blocks [0, nblk) contiguously, one or more blocks each, tiles after the first starting at
 * block 2 or later, in any order in the table, with part = the wave's first record + the segment's index
 * and the same nseg in each. */
/* Host-side planner, no device call; d_in and d_out are used as addresses only (alignment class).
 * seg_blocks == 0: the segment length cz_engine_flush_in picks for a flush of the call's total body
 * bytes.  Every refusal of cz_plan_fanin applies, checked before anything is written; more than 2^32 - 1
 * tiles, join waves or partial records: CZ_EINVAL.  *ntiles = sum over runs of segments x
 * ceil(count / 64), *njoins = sum over split runs of ceil(count / 64), *npart = sum over split runs of
 * count x segments (d_work must hold 64 bytes each).  A tile_cap / join_cap below that (or a null table)
 * returns CZ_EINVAL with the three sizes set and nothing else written, as cz_plan_fanout_split.
 * class_count[c] = tiles of class c; inside a class the tiles with the most output chunks come first.
 * Replaces StreamEngine.decodeAndPush -> mechanism.decode, once per message and per connection
 * (StreamEngine.java:1067-1098, CurveClientMechanism.java:166-224, CurveServerMechanism.java:165-225). */
int cz_plan_fanin_split(const cz_fanin_run *h_runs, uint32_t nruns, const void *d_in, const void *d_out,
                        uint32_t seg_blocks, cz_fanout_tile *h_tiles, uint32_t tile_cap, uint32_t *ntiles,
                        uint32_t class_count[2], cz_fanout_join *h_joins, uint32_t join_cap, uint32_t *njoins,
                        uint32_t *npart);
/* StreamEngine.decodeAndPush -> mechanism.decode, once per message and per connection
 * (StreamEngine.java:1067-1098, CurveClientMechanism.java:166-224, CurveServerMechanism.java:165-225):
 * all of it for R runs, in at most three launches whatever R (tiles of the line class, lane-wise tiles,
 * join).  d_runs / d_tiles / d_joins: device copies of the run array and of the planner's tables;
 * class_count as the planner returned it.  Asynchronous on `stream`; allocates nothing; never
 * synchronises; can be captured into a graph.  nruns == 0 or no tiles: CZ_OK, nothing launched.  Null
 * pointers (d_joins / d_work only when njoins != 0; d_nonces is optional): CZ_EINVAL, checked before the
 * device is touched.  No device: CZ_EHIP; there is no CPU fallback. */
int cz_open_fanin_split(const cz_fanin_run *d_runs, uint32_t nruns, const cz_fanout_tile *d_tiles,
                        const uint32_t class_count[2], const cz_fanout_join *d_joins, uint32_t njoins,
                        const void *d_in, const cz_fanin_sub *d_subs, const void *d_subkeys, void *d_out,
                        void *d_work, uint16_t *d_status, uint64_t *d_nonces, void *stream);

/* ---- 3h. relay: received bodies re-sealed for another peer in one launch ---------------------
 * What a broker does with most of its traffic: a frame arrives under connection A's key and leaves
 * under connection B's key and nonce.  Replaces Proxy.forward (zmq/Proxy.java:140-160: from.recv, then
 * to.send) -> CurveServerMechanism.decode (CurveServerMechanism.java:165-225) / CurveClientMechanism.decode
 * (CurveClientMechanism.java:165-224) on one StreamEngine -> encode (:126-163) on another.  With sections
 * 3 above that is cz_open_batch, which writes the plaintext to device memory, and cz_seal_batch, which
 * reads it back.  A re-sealed MESSAGE body has exactly the size and layout of the received one
 * ("\x07MESSAGE" | nonce8 | tag16 | c), and from box byte 32 on c_out = c_in ^ ks_in ^ ks_out: one pass,
 * one load stream and one store stream, the authenticated plaintext in registers only, and the V2
 * header in front of the body stays valid (size and MORE are unchanged).
 *
 * ACCEPTED FRAME: the output is, byte for byte, what Mechanism.encode produces for the Msg that
 * Mechanism.decode delivers: the payload unchanged, the flags byte decrypted_flags & (CZ_MSG_MORE |
 * CZ_MSG_COMMAND) -- the reference keeps only these two bits through a Msg
 * (CurveServerMechanism.java:207-213 and :132-138) --, the outbound nonce and the tag under the
 * outbound subkey.  REJECTED FRAME (any status but CZ_STATUS_OK): its `len` / `size` output bytes are
 * written as zero -- a COMMAND, MALFORMED or SEQUENCE frame is rejected before decryption; a bad tag
 * is found after the body was emitted and its bytes are overwritten before the kernel ends.  A zero
 * body cannot parse as MESSAGE: no sealed copy of unauthenticated plaintext is ever left in d_out.
 *
 * cz_relay_batch: one lane per frame, no new record types.  d_desc[i] is read exactly as cz_open_batch
 * reads it (in_off, len = the body size, key_idx = the inbound subkey, counter = the floor,
 * CZ_DESC_CHECK_NONCE, prev); out_off is where the re-sealed body of the same len bytes goes.  d_to[i]
 * is the cz_fanout_sub {counter, key_idx} of section 3c: the outbound cnNonce and the outbound subkey
 * in the same table.  Inbound and outbound key, and inbound and outbound counter, may be equal.
 * Input and output at any byte alignment, independently of each other.  d_order as in cz_open_batch.
 * d_status[i] and d_nonces[i] (optional) are exactly cz_open_batch's: the full decrypted flags byte in
 * bits 8..15 of an OK status, and the inbound wire nonce.  len == 0 writes nothing.
 * IN PLACE: d_out + out_off == d_in + in_off is legal for a frame with prev < 0 (the lane reads the
 * header, the tag and each block before it stores over them).  With prev >= 0 an in-place relay is
 * the caller's error: the floor would be read from a body another lane may already have re-sealed.
 * Any other overlap of input and output ranges is the caller's error too.
 * Null pointers (d_order and d_nonces are optional): CZ_EINVAL, checked before the device is touched.
 * count == 0: CZ_OK, nothing launched.  No device: CZ_EHIP; there is no CPU fallback.  Asynchronous on
 * `stream`; allocates nothing; can be captured into a graph. */
int cz_relay_batch(const cz_frame_desc *d_desc, const cz_fanout_sub *d_to, const uint32_t *d_order, uint32_t count,
                   const void *d_in, void *d_out, const void *d_subkeys, uint16_t *d_status, uint64_t *d_nonces,
                   void *stream);
/* One connection's bodies forwarded to one connection, the throughput form (a streamer, one backend):
 * `count` bodies of `size` bytes at d_in + i * in_stride, re-sealed to d_out + i * out_stride.  Replaces
 * the same Proxy.forward -> decode -> encode path (Proxy.java:140-160, CurveServerMechanism.java:165-225 /
 * CurveClientMechanism.java:165-224, :126-163), once per message.
 * CHAIN: cz_open_uniform's rule -- frame 0 must beat floor0, frame i the wire nonce of frame i - 1,
 * whether that frame was accepted or not (when check != 0).  d_status[i] as cz_open_uniform.
 * COUNTERS: frame i is re-sealed with nonce counter0 + i (mod 2^64, as cz_seal_uniform).  A rejected
 * frame still consumes its counter: the outbound stream then has a gap, which a CURVE receiver
 * accepts because it asks only for a strictly increasing nonce (CurveClientMechanism.java:186-193).
 * OUTPUT OWNERSHIP by out_stride alone, the rule of cz_seal_uniform: an owning stride gets zeros past
 * each body and over a rejected frame's whole slot; any other stride writes only the `size` bytes of
 * each body, as zeros when the frame is rejected.  size < 33: every frame is COMMAND or MALFORMED and
 * only zeros are written.
 * Input and output ranges must not overlap: there is no in-place here (the line stores of a body are
 * issued by other lanes).  Full waves of bodies of at least 256 bytes with d_in, in_stride, d_out and
 * out_stride on 16 bytes and out_stride a multiple of 128 below 32 MiB store whole lines; every other
 * layout (the dense stride 4129, the last partial wave) is stored lane by lane, byte-exact.
 * Null pointers: CZ_EINVAL before the device is touched; count == 0: CZ_OK; no device: CZ_EHIP, no CPU
 * fallback; asynchronous on `stream`, allocates nothing, can be captured into a graph. */
int cz_relay_uniform(uint32_t count, uint32_t size, const void *d_in, uint64_t in_stride, void *d_out,
                     uint64_t out_stride, const void *d_subkey_in, uint64_t floor0, int check,
                     const void *d_subkey_out, uint64_t counter0, uint16_t *d_status, void *stream);

/* ---- 3i. segmented relay: long received bodies re-sealed across lanes ------------------------
 * cz_relay_batch keeps a whole frame on one lane: a 64 KiB body is 1025 blocks of double work (two
 * keystreams, two Poly1305 chains) and a ragged batch waits for its longest frame.  This call is the
 * relay of section 3h on the segment plan of section 3b: one lane per segment, then one combine lane
 * per split frame.  It replaces the same reference path, Proxy.forward (zmq/Proxy.java:140-160) ->
 * Mechanism.decode (CurveServerMechanism.java:165-225 / CurveClientMechanism.java:165-224) ->
 * Mechanism.encode (:126-163), once per message.
 *
 * d_desc[i] and d_to[i] are read exactly as cz_relay_batch reads them (len = the body size, out_off =
 * where the re-sealed body of the same size goes, prev chains allowed).  THE PLAN is the one
 * cz_plan_segments(h_desc, count, open = 1, seg_blocks, ...) makes for those descriptors -- the plan a
 * cz_open_segments of them would take; there is no planner and no record type of its own.  A caller may
 * build its own plan under section 3b's rule: the segments of a split frame cover box blocks [0, nblk)
 * contiguously, one or more blocks each, with consecutive part indices from the frame's part0, in any
 * order in the list.  The open's "block 2 or later" rule is NOT needed here (block q in gives block q
 * out: a segment's output is its own blocks' bytes); plans that obey it work as well.
 * WORKSPACE: d_work holds 128 bytes per part, two planes of npart 64-byte records: the inbound Poly1305
 * partial of part p is record p (cz_open_segments' record, with the flags byte and the early status
 * from the segment holding block 0), the outbound partial is record npart + p.  d_comb and d_work are
 * needed only when ncomb != 0.
 * OUTPUT, byte for byte what cz_relay_batch writes for the same d_desc and d_to: the bodies,
 * d_status[i] and d_nonces[i] (optional).  Every rejected frame's len output bytes are written as zero;
 * nothing outside the bodies, and no status or nonce entry of another frame, is touched.  A frame
 * rejected before decryption (COMMAND, MALFORMED, SEQUENCE): each of its segments zeroes its own byte
 * range, the segment holding block 0 writes the status and the nonce.  A bad tag on a split frame is
 * found by the combine lane, which zeroes the whole body and writes CZ_STATUS_CRYPTO: no sealed copy of
 * unauthenticated plaintext is left in d_out once the call's last kernel has finished.
 * NO IN PLACE: input and output ranges must not overlap (later segments re-read the header nonce, and
 * the combine re-reads the inbound tag, after the first segment may already have stored).
 * Full waves of segments with one block count, bodies and outputs on 16 bytes and no rejected frame
 * store whole lines; every other wave stores lane by lane, byte-exact at any alignment of either side.
 * Null pointers (d_nonces is optional; d_comb and d_work only with ncomb != 0): CZ_EINVAL before the
 * device is touched.  nseg == 0: CZ_OK, nothing launched.  No device: CZ_EHIP; there is no CPU
 * fallback.  Asynchronous on `stream`, allocates nothing, never synchronises, can be captured into a
 * graph; at most two launches (segments, then combine). */
int cz_relay_segments(const cz_frame_desc *d_desc, const cz_fanout_sub *d_to, const cz_segment *d_seg, uint32_t nseg,
                      const cz_combine *d_comb, uint32_t ncomb, uint32_t npart, const void *d_in, void *d_out,
                      const void *d_subkeys, void *d_work, uint16_t *d_status, uint64_t *d_nonces, void *stream);

/* Synthetic data: fill d_buf with the counter-based SplitMix64 byte stream (seed). */
int cz_fill(void *d_buf, uint64_t nbytes, uint64_t seed, void *stream);
/* Measurement: device-to-device copy of nbytes (a multiple of 16) with 16-byte loads and stores,
 * the float4 copy the MI355X guide measures at 6.29 TB/s; bench.py's HBM copy ceiling. */
int cz_dev_copy(void *d_dst, const void *d_src, uint64_t nbytes, void *stream);

/* ---- 4. host-staged batches (the JNI path: Java byte[] / direct ByteBuffer) -------
 * A context owns a HIP stream, pinned host staging and device buffers that grow
 * on demand.  cz_ctx_seal/open copy host frames in, run the batch kernel and copy
 * the results out (synchronous).  These are what a JNI shim binds. */
typedef struct cz_ctx cz_ctx;
int cz_ctx_create(cz_ctx **out, int device);
void cz_ctx_destroy(cz_ctx *ctx);
/* upload `nkeys` 32-byte cnPrecom keys and derive their subkeys for `direction` */
int cz_ctx_set_keys(cz_ctx *ctx, const uint8_t *h_precom, uint32_t nkeys, int direction);
int cz_ctx_seal(cz_ctx *ctx, const cz_frame_desc *h_desc, uint32_t count, const void *h_in, uint64_t in_bytes,
                void *h_out, uint64_t out_bytes);
int cz_ctx_open(cz_ctx *ctx, const cz_frame_desc *h_desc, uint32_t count, const void *h_in, uint64_t in_bytes,
                void *h_out, uint64_t out_bytes, uint16_t *h_status);
/* Pipelined host-staged uniform batches (the end-to-end path at throughput): frames in
 * chunks of chunk_frames (0 = 16384); chunk k runs H2D -> kernel
 * -> D2H on one of three streams with its own device buffers, so PCIe copies in both
 * directions overlap each other and the kernels.  A batch that is one chunk of at most
 * 64 MiB (in + out slots) of frames of 8+ blocks runs on one stream through the segment
 * kernels instead, so a few frames cost tens of us rather than one lane's whole walk.  Both
 * paths write whole output slots: each body followed by zeros to the end of its slot, and
 * zeros in the payload slot of a rejected open, whatever the batch size or chunk_frames.
 * For count == 1 the strides are ignored and the slot is the body alone.  Host buffers
 * should be pinned (cz_host_alloc) for full PCIe rate; the output host buffer must span
 * count * out_stride bytes (whole slots).  Uses the
 * context's key 0 (cz_ctx_set_keys).  Synchronous. */
int cz_ctx_seal_uniform(cz_ctx *ctx, uint32_t count, uint32_t len, const void *h_in, uint64_t in_stride, void *h_out,
                        uint64_t out_stride, uint64_t counter0, const uint8_t *h_flags8, uint32_t chunk_frames);
int cz_ctx_open_uniform(cz_ctx *ctx, uint32_t count, uint32_t size, const void *h_in, uint64_t in_stride, void *h_out,
                        uint64_t out_stride, uint64_t floor0, int check, uint16_t *h_status, uint32_t chunk_frames);
/* pinned host buffers for zero-extra-copy callers (a pinned MsgAllocator, zmq/msg/MsgAllocator.java:5-8).
 * cz_host_free frees only a base address cz_host_alloc returned and not yet freed (CZ_OK); any
 * other pointer -- an interior address, foreign memory, a second free -- is CZ_EINVAL and left alone. */
void *cz_host_alloc(uint64_t bytes);
int cz_host_free(void *p);

/* ---- 5. CURVE mechanism objects (host mirror of CurveClientMechanism / CurveServerMechanism
 *         in the CONNECTED state: encode/decode of MESSAGE commands with nonce bookkeeping) ---- */
typedef struct cz_mech cz_mech;
/* as_server = 0: client (seals ...MESSAGEC, opens ...MESSAGES); 1: server.
 * cn_nonce / cn_peer_nonce: the handshake's final values (client
 * MESSAGEs start at 3, server at 2). */
cz_mech *cz_mech_create(int as_server, const uint8_t precom[32], uint64_t cn_nonce, uint64_t cn_peer_nonce,
                        int device);
void cz_mech_destroy(cz_mech *m);
/* encode one Msg: out must hold n + 33 bytes; returns the body length or a negative CZ_E* */
int64_t cz_mech_encode(cz_mech *m, const uint8_t *payload, uint64_t n, int msg_flags, uint8_t *out);
/* decode one body: returns the payload length (>= 0) and *msg_flags, or CZ_EPROTO with
 * *event = ZMQ_PROTOCOL_ERROR_* code (zmq/ZMQ.java:209-227) the reference would raise */
int64_t cz_mech_decode(cz_mech *m, const uint8_t *body, uint64_t size, uint8_t *out, int *msg_flags, int *event);
/* batched encode of count frames packed back to back: payloads at in_off[i] (len[i]),
 * bodies written at out_off[i].  One device launch for the whole batch. */
int cz_mech_encode_batch(cz_mech *m, uint32_t count, const uint8_t *h_in, const uint64_t *in_off,
                         const uint32_t *len, const uint8_t *msg_flags, uint8_t *h_out, const uint64_t *out_off);
/* batched decode: stops at the first failing frame like StreamEngine does (returns its index
 * in *failed, or -1); frames before it are delivered. */
int cz_mech_decode_batch(cz_mech *m, uint32_t count, const uint8_t *h_in, const uint64_t *in_off,
                         const uint32_t *size, uint8_t *h_out, const uint64_t *out_off, uint8_t *msg_flags,
                         int32_t *failed, int *event);
uint64_t cz_mech_nonce(const cz_mech *m);
uint64_t cz_mech_peer_nonce(const cz_mech *m);

/* ZMTP protocol-error event codes (zmq/ZMQ.java:214-227) */
#define CZ_ZMTP_UNEXPECTED_COMMAND 0x10000001
#define CZ_ZMTP_MALFORMED_COMMAND_MESSAGE 0x10000012
#define CZ_ZMTP_INVALID_SEQUENCE 0x10000002
#define CZ_ZMTP_CRYPTOGRAPHIC 0x11000001
#define CZ_ZMTP_UNSPECIFIED 0x10000000
#define CZ_ZMTP_KEY_EXCHANGE 0x10000003
#define CZ_ZMTP_MALFORMED_COMMAND_HELLO 0x10000013
#define CZ_ZMTP_MALFORMED_COMMAND_INITIATE 0x10000014
#define CZ_ZMTP_MALFORMED_COMMAND_ERROR 0x10000015
#define CZ_ZMTP_MALFORMED_COMMAND_READY 0x10000016
#define CZ_ZAP_MALFORMED_REPLY 0x20000001
#define CZ_ZAP_INVALID_STATUS_CODE 0x20000004

/* ---- 7. ZMTP v2 framing (zmq/io/coder/v2/V2Encoder.java, V2Decoder.java) ----------------
 * Wire frame = flags byte (MORE 1, LARGE 2, COMMAND 4: V1Protocol/V2Protocol) + size
 * (1 byte, or BE64 with LARGE when size > 255: V2Encoder.java:31-55) + body. */
#define CZ_V2_MORE 0x01
#define CZ_V2_LARGE 0x02
#define CZ_V2_COMMAND 0x04
/* header bytes V2Encoder writes before a body of `size` bytes: 2, or 9 when size > 255 */
uint32_t cz_v2_header_size(uint64_t size);
/* Host parser with V2Decoder's rules (V2Decoder.java:37-105, Decoder.java:76-98): parses whole
 * frames from wire[0:len) into frames[] (body offset, size, Msg flags MORE=CZ_MSG_MORE /
 * COMMAND=CZ_MSG_COMMAND), stopping at cap frames or at an incomplete frame.  *consumed = bytes
 * of the whole frames.  Returns CZ_OK, or CZ_EPROTO (LARGE size <= 0 as a signed long) /
 * CZ_EMSGSIZE (size > maxmsgsize >= 0, or > INT32_MAX) at the first bad header; the frames
 * before it are still reported.  No device needed. */
typedef struct cz_v2_frame {
    uint64_t body_off;
    uint32_t size;
    uint32_t msg_flags;
} cz_v2_frame;
int cz_v2_parse(const uint8_t *wire, uint64_t len, int64_t maxmsgsize, cz_v2_frame *frames, uint32_t cap,
                uint32_t *nframes, uint64_t *consumed);
/* Device: one copy per item, any byte alignment.  With CZ_V2_ITEM_HEADER in flags, the V2
 * header for `size` (wire flags = flags & 0xff, LARGE set by size) is written at dst_off and the
 * body after it: packing sealed MESSAGE bodies into socket-ready wire streams.  Without it a
 * plain copy: unpacking received bodies into aligned slots for the open kernels. */
#define CZ_V2_ITEM_HEADER 0x100
typedef struct cz_v2_item {
    uint64_t src_off;
    uint64_t dst_off;
    uint32_t size;
    uint32_t flags;
} cz_v2_item;
int cz_v2_copy(const cz_v2_item *d_items, uint32_t count, const void *d_src, void *d_dst, void *stream);

/* ---- 7b. device V2 scan: many received streams parsed where they lie ------------------------
 * The decode half of section 7 for the many-connection shape: `count` received streams in device
 * memory, one lane per stream walking its own header chain with cz_v2_parse's rules bit for bit
 * (V2Decoder.java:37-105, Decoder.java:76-98), no frame capacity.  A stream is bytes
 * [off, off + len) of d_wire at any byte alignment; headers are read with aligned dword loads that
 * never touch a dword holding no byte of the stream. */
typedef struct cz_v2_stream {        /* 32 bytes */
    uint64_t off, len;               /* received bytes in d_wire */
    uint64_t floor;                  /* cnPeerNonce: replay floor of the stream's first frame */
    uint32_t key_idx, reserved;
} cz_v2_stream;
typedef struct cz_v2_stream_result { /* 32 bytes */
    uint64_t consumed, slot_off;     /* bytes of the whole frames; where the stream's plaintext slots start */
    uint32_t first, nframes;         /* the stream's frames are records [first, first + nframes) */
    int32_t rc; uint32_t reserved;   /* CZ_OK / CZ_EPROTO / CZ_EMSGSIZE, as cz_v2_parse returns */
} cz_v2_stream_result;
typedef struct cz_v2_totals { uint64_t nframes, slot_bytes; } cz_v2_totals;
/* Scan + placement (V2Decoder.java:37-105 / Decoder.java:76-98): per stream nframes, consumed and rc as
 * cz_v2_parse gives them, and first / slot_off = the exclusive sums over the streams of nframes and of the
 * plaintext slot bytes, sum of round_up(max(size - 33, 1), slot_align) with size - 33 taken as 0 below 33;
 * *d_totals = the two sums.  slot_align: a power of two from 1 to 4096.  count == 0: CZ_OK, zero totals. */
int cz_v2_scan(const cz_v2_stream *d_streams, uint32_t count, const void *d_wire, int64_t maxmsgsize,
               uint32_t slot_align, cz_v2_stream_result *d_results, cz_v2_totals *d_totals, void *stream);
/* Emit (the frames V2Decoder.java:37-105 / Decoder.java:76-98 would hand on): repeats the walk over the
 * frames d_results counted and writes, for frame k of stream s at index first + k, a cz_v2_frame {body_off
 * relative to the stream, size, msg_flags} and / or the open's descriptor {in_off = off + body_off, out_off =
 * its slot, len = size, key_idx, counter = floor, flags = CZ_DESC_CHECK_NONCE, prev = k ? index - 1 : -1}.
 * Nothing is written at or past first + nframes.  Either output may be NULL. */
int cz_v2_scan_emit(const cz_v2_stream *d_streams, const cz_v2_stream_result *d_results, uint32_t count,
                    const void *d_wire, uint32_t slot_align, cz_v2_frame *d_frames, cz_frame_desc *d_desc,
                    void *stream);                       /* either output may be NULL */
/* V2Decoder.java:37-105 / Decoder.java:76-98 + Mechanism.decode for every whole frame of every stream:
 * scan, read the totals (one synchronisation), emit, cz_open_batch from the wire bytes where they lie.
 * CZ_ENOMEM with *h_totals filled and nothing opened when the totals exceed desc_cap / out_cap;
 * CZ_EINVAL above 2^31 - 1 frames.  d_status / d_nonces (optional) hold desc_cap records.  A frame's
 * replay floor is read at bytes [8, 16) of the frame before it even when that frame is shorter, so
 * d_wire must be readable for 16 bytes past its last stream. */
int cz_open_streams(const cz_v2_stream *d_streams, uint32_t count, const void *d_wire, int64_t maxmsgsize,
                    uint32_t slot_align, cz_v2_stream_result *d_results, cz_frame_desc *d_desc, uint64_t desc_cap,
                    void *d_out, uint64_t out_cap, const void *d_subkeys, uint16_t *d_status, uint64_t *d_nonces,
                    cz_v2_totals *h_totals, void *stream);

/* ---- 3j. stream relay: received V2 streams re-sealed wire to wire (placed here for section 7b's records) ----
 * Sections 3h and 7b together, for a broker's received byte streams.  A re-sealed body has the size and layout
 * of the received one, so the V2 header in front of it stays valid: a received wire stream whose bodies are
 * re-sealed where they lie IS the outbound wire stream.  Replaces Proxy.forward (zmq/Proxy.java:140-160) per
 * message: V2Decoder (V2Decoder.java:37-105, Decoder.java:76-98) and Mechanism.decode
 * (CurveServerMechanism.java:165-225 / CurveClientMechanism.java:165-224) on one StreamEngine, Mechanism.encode
 * (:126-163) and V2Encoder (V2Encoder.java:31-55) on another.
 *
 * d_streams[s] is section 7b's record (bytes, floor, inbound key).  d_to[s] = {counter, key_idx}: the outbound
 * cnNonce of the stream's first frame and the outbound subkey.  Frame k of the stream is sealed with counter + k
 * (mod 2^64); a rejected frame consumes its counter, cz_relay_uniform's rule (the receiver accepts the gap:
 * CurveClientMechanism.java:186-193).  Inbound and outbound key and counter may be equal.
 * THE CHAIN, as cz_open_streams: scan (slot_off / slot_bytes of d_scan and *h_totals mean nothing here), one
 * synchronisation to read *h_totals, then on `stream` with no further synchronisation: emit -- for frame k of
 * stream s at index i = first + k, d_desc[i] = {in_off = out_off = the body's offset, len, key_idx, counter =
 * the frame's replay floor, CZ_DESC_CHECK_NONCE, prev = -1} and d_to_frames[i] = {counter + k, key_idx} --,
 * cz_relay_batch over those nframes descriptors, and the cut.  The floor of frame k > 0 is the big-endian u64
 * at bytes [8, 16) of frame k - 1's body, read by the emit before the relay stores anything: that is what makes
 * the relay legal in place under 3h's rule.  It is read even when that body is shorter than 16 bytes, so d_wire
 * must be readable for 16 bytes past its last stream (cz_open_streams' rule).
 * d_out == d_wire: in place.  Otherwise d_out must not overlap d_wire and takes the same offsets; the 2 or 9
 * header bytes of every whole frame are copied over byte-exact.  No byte of d_out outside the headers and bodies
 * of whole frames is written: not a trailing partial frame, not the bytes between streams.
 * d_status[i] / d_nonces[i]: cz_relay_batch's.  An accepted body is, byte for byte, Mechanism.encode's output for
 * the Msg Mechanism.decode delivers; a rejected frame's body is zeros (3h).
 * d_results[s]: what of the stream may leave.  Frames behind the first rejected one were relayed by their own
 * lanes and may sit sealed in d_out: A CALLER SENDS ok_bytes (OR whole_bytes) OF A STREAM AND NOTHING BEHIND THEM.
 * peer_nonce is cnPeerNonce after the stream by the engine's delivery rule: the wire nonce of the last accepted
 * frame; the rejected frame's when fail_status == CZ_STATUS_CRYPTO (its nonce passed the replay check before
 * the tag failed: CurveClientMechanism.java:193); the stream's floor when neither applies.
 * CZ_ENOMEM with *h_totals filled and nothing written to d_out when nframes > desc_cap (d_desc, d_to_frames,
 * d_status and d_nonces hold desc_cap records each); CZ_EINVAL above 2^31 - 1 frames.  Null pointers (all are
 * required, d_nonces included): CZ_EINVAL before the device is touched.  count == 0: CZ_OK, zero totals.  No
 * device: CZ_EHIP; there is no CPU fallback.  Every frame is one lane of the relay: long frames are correct but
 * slow. */
typedef struct cz_relay_stream_result {   /* 32 bytes */
    uint64_t ok_bytes;      /* wire bytes (headers + bodies) of the frames before the first rejected one */
    uint64_t whole_bytes;   /* <= ok_bytes: cut back to the end of the last frame whose decrypted flags lack MORE */
    uint64_t peer_nonce;    /* cnPeerNonce after the stream */
    uint32_t ok_frames;
    uint16_t fail_status;   /* CZ_STATUS_* of the first rejected frame, CZ_STATUS_OK when none */
    uint16_t reserved;      /* 0 */
} cz_relay_stream_result;
int cz_relay_streams(const cz_v2_stream *d_streams, const cz_fanout_sub *d_to, uint32_t count,
                     const void *d_wire, void *d_out, int64_t maxmsgsize,
                     cz_v2_stream_result *d_scan, cz_frame_desc *d_desc, cz_fanout_sub *d_to_frames,
                     uint64_t desc_cap, const void *d_subkeys, uint16_t *d_status, uint64_t *d_nonces,
                     cz_relay_stream_result *d_results, cz_v2_totals *h_totals, void *stream);

/* ---- 8. batching engine: many CURVE connections, one device batch per flush -----------------
 * The GPU form of StreamEngine's encode/decode loops (outEvent: pull + mechanism.encode +
 * V2Encoder up to OUT_BATCH_SIZE, StreamEngine.java:467-535; inEvent: V2Decoder +
 * mechanism.decode, :379-465, decodeAndPush :1067-1098) across connections: messages of all
 * connections are sealed in one segmented device batch and packed into per-connection wire
 * streams; received wire bytes of all connections are parsed, opened in one batch and checked
 * against each connection's nonce chain.  Payload buffers come from a pinned arena
 * (ZMQ_MSG_ALLOCATOR, zmq/msg/MsgAllocator.java:5-8).  Not thread-safe: one engine per thread. */
typedef struct cz_engine cz_engine;
/* arena_bytes: capacity of the pinned outbound payload arena (messages per flush) */
int cz_engine_create(cz_engine **e, uint64_t arena_bytes, int device);
void cz_engine_destroy(cz_engine *e);
/* returns a connection id >= 0; cn_nonce / cn_peer_nonce as cz_mech_create */
int cz_engine_add_conn(cz_engine *e, int as_server, const uint8_t precom[32], uint64_t cn_nonce,
                       uint64_t cn_peer_nonce);
/* the connection is gone (StreamEngine unplug / error, StreamEngine.java:334-370,1116-1131): its
 * queued messages are dropped from the next flush, its received bytes and last flush_in payloads
 * are discarded, its subkeys are wiped, and its id is reused by a later cz_engine_add_conn.
 * Every other call on the id fails with CZ_EINVAL until then. */
int cz_engine_remove_conn(cz_engine *e, int conn);
/* pinned payload buffer inside the arena (no copy at send); NULL when the arena is full */
void *cz_engine_msg_alloc(cz_engine *e, uint32_t len);
/* queue one Msg (payload from cz_engine_msg_alloc, or copied into the arena); CZ_ENOMEM when the
 * arena is full (flush first), CZ_EPROTO when the connection has failed */
int cz_engine_send(cz_engine *e, int conn, const void *payload, uint32_t len, int msg_flags);
/* PUB fan-out (Dist.distribute, zmq/socket/pubsub/Dist.java): queue ONE Msg for each of the nconn
 * listed connections, in list order, at this point of the send order.  The payload is staged in
 * the arena once (or not at all when it already lies there), so N subscribers cost len arena
 * bytes, not N * len; a multipart message is several calls with CZ_MSG_MORE.  Everything is
 * checked before anything is queued: an unknown or removed id is CZ_EINVAL, an over-long payload
 * CZ_EMSGSIZE, a full arena CZ_ENOMEM, each with nothing queued.  Connections that have failed
 * are skipped (Dist.write drops a pipe it cannot write to); *queued (optional) = frames queued.
 * An id listed twice gets two frames with consecutive nonces.  flush_out takes a publish's run
 * of at least cz_tune("fanout_min") frames -- or of at least 64 frames with a payload of at most
 * cz_tune("fanout_short") bytes -- out of the segment plan, and seals all such runs of a flush
 * group with one cz_seal_fanout_runs call.  Every other run of at least 64 frames whose payload is
 * at least cz_tune("fanout_split") bytes leaves the segment plan too, for the group's one
 * cz_seal_fanout_split call at the flush's own segment length.  The wire bytes are those
 * of the same messages queued with cz_engine_send, whichever way the frames are routed. */
int cz_engine_publish(cz_engine *e, const int *conns, uint32_t nconn, const void *payload, uint32_t len,
                      int msg_flags, uint32_t *queued);
/* seal every queued Msg on the device and V2-frame it into one pinned output in SEND order
 * (valid until the next cz_engine_flush_out).  The flush is pipelined in groups of ~8 MiB+:
 * H2D of a group overlaps the seal + D2H of the one before. */
int cz_engine_flush_out(cz_engine *e);
/* one connection's MESSAGE frames, in its send order, as contiguous bytes: a pointer into the
 * flush output when its messages were queued back to back, else a host-gathered copy */
int cz_engine_wire_out(cz_engine *e, int conn, const uint8_t **wire, uint64_t *len);
/* the same stream as gather-write pieces of the flush output (for writev / a GatheringByteChannel,
 * StreamEngine.java:509-535): *count = pieces; fills iov when cap >= *count (cap 0: count only) */
typedef struct cz_iovec {
    const uint8_t *base;
    uint64_t len;
} cz_iovec;
int cz_engine_wire_iov(cz_engine *e, int conn, cz_iovec *iov, uint32_t cap, uint32_t *count);
/* append bytes received on a connection (partial frames are kept for the next flush) */
int cz_engine_recv(cz_engine *e, int conn, const void *wire, uint64_t len);
/* zero-copy receive (the V2Decoder getBuffer() pattern, StreamEngine.java:403-410): a pinned
 * buffer of *avail >= min_bytes bytes at the end of the connection's received data; read from
 * the socket into it, then commit the bytes read.  Valid until the next engine call. */
int cz_engine_recv_buffer(cz_engine *e, int conn, uint64_t min_bytes, uint8_t **buf, uint64_t *avail);
int cz_engine_recv_commit(cz_engine *e, int conn, uint64_t n);
/* parse, open and sequence-check every whole frame received on every connection.  Inside a flush
 * group (connection by connection, each connection's frames in order) a run of at least 64 consecutive
 * frames of one body size whose payload is at most cz_tune("fanin_short") bytes leaves the segment plan,
 * and all such runs of the group are one cz_open_fanin_runs call (section 3f); a run may span
 * connection edges.  Every other such run whose payload is at least cz_tune("fanin_split") bytes leaves
 * the segment plan too, for the group's one cz_open_fanin_split call (section 3g) at the flush's own
 * segment length; a run cut by a group edge is two runs.  Delivered messages, cnPeerNonce, errors and
 * events are those of the unrouted flush. */
int cz_engine_flush_in(cz_engine *e);
/* frames of the last cz_engine_flush_in that its cz_open_fanin_runs calls opened (0: nothing was routed) */
uint64_t cz_engine_fanin_frames(const cz_engine *e);
/* ... and that its cz_open_fanin_split calls opened */
uint64_t cz_engine_fanin_split_frames(const cz_engine *e);
/* Scanned flush (section 7b), cz_tune("scan_in") = n > 0 bytes: a flush in which at least 64 live connections
 * have received bytes and every one of them holds at most n takes no host parse at all.  The received bytes
 * go over as in any flush, one 32-byte cz_v2_stream per connection follows, the device scans and places them,
 * the totals come back (the flush's one extra synchronisation), and cz_v2_scan_emit's descriptors open every
 * frame from the wire bytes where they lie: no unpacking copy, no per-frame metadata upload, no segment plan
 * and no fan-in routing.  Always one group.  Delivered messages, cnPeerNonce, errors and events are those of
 * the unscanned flush.  Frames of the last cz_engine_flush_in opened this way (0: the path was not taken): */
uint64_t cz_engine_scan_frames(const cz_engine *e);
/* Forward routes (section 3j), the broker's Proxy.forward (zmq/Proxy.java:140-160: from.recv, then to.send --
 * V2Decoder.java:37-105 / Decoder.java:76-98, Mechanism.decode CurveServerMechanism.java:165-225 /
 * CurveClientMechanism.java:165-224, Mechanism.encode :126-163) without the plaintext ever reaching memory:
 * everything `from` receives leaves re-sealed for `to`.  ONE SOURCE PER DESTINATION: CZ_EINVAL for an unknown or
 * removed id, for from == to, and for a `to` that another live route already names; A -> B together with B -> A
 * is the normal proxy and is legal.  to = -1 clears the route of `from`; removing either end clears it too.
 * cz_engine_flush_in skips a connection that has a route: its bytes wait for cz_engine_flush_forward. */
int cz_engine_forward(cz_engine *e, int from, int to);
/* Every route whose source holds received bytes, in one chain on one stream: the received bytes go over as they
 * lie with one cz_v2_stream and one cz_fanout_sub per route, cz_relay_streams' chain runs IN PLACE (headers
 * kept), and the wire bytes and the 32-byte cz_relay_stream_result per route come back into pinned memory: no
 * per-frame metadata crosses PCIe in either direction.  CUT AT THE FIRST REJECTED FRAME: a route's ok_bytes leave
 * and nothing behind them; the source then fails exactly as in cz_engine_flush_in (CZ_EPROTO, the event of the
 * rejected frame's status, its received bytes dropped), and a framing error behind good frames gives the framing
 * error with event 0.  Otherwise the whole frames leave the receive buffer and a partial frame stays.  The
 * source's cnPeerNonce becomes the result's peer_nonce; the destination's cnNonce advances by the frames
 * scanned, as every one consumed a counter.  A route whose destination has failed leaves the source's bytes where
 * they are and forwards nothing.  cz_engine_flush_out assigns nonces when it runs, so the one ordering rule is:
 * bytes go to the destination's socket in the order of the flush calls that produced them. */
int cz_engine_flush_forward(cz_engine *e);
/* the bytes the last cz_engine_flush_forward made for the destination of `from`'s route: socket-ready wire
 * frames in pinned memory, valid until the next cz_engine_flush_forward (*len 0: nothing to send) */
int cz_engine_forward_out(cz_engine *e, int from, const uint8_t **wire, uint64_t *len);
/* frames the last cz_engine_flush_forward forwarded (the frames inside every route's ok_bytes) */
uint64_t cz_engine_forward_frames(const cz_engine *e);
/* decoded messages of the last cz_engine_flush_in (pinned memory, valid until the next one) */
int cz_engine_msgs_in(cz_engine *e, int conn, uint32_t *count);
int cz_engine_msg_in(cz_engine *e, int conn, uint32_t i, const uint8_t **payload, uint32_t *len, int *msg_flags);
/* 0 while the connection is healthy; after a failure CZ_EPROTO / CZ_EMSGSIZE and *event = the
 * ZMTP protocol-error event the reference raises (0 for a framing error) */
int cz_engine_conn_error(cz_engine *e, int conn, int *event);
uint64_t cz_engine_nonce(cz_engine *e, int conn);
uint64_t cz_engine_peer_nonce(cz_engine *e, int conn);

/* ---- 9. handshake public-key calls (Curve.java:84-193 -> jnacl) --------------------------
 * jnacl int contract (0 / -1).  X25519 per RFC 7748 on the device; box / box_open are
 * beforenm + the section-1 afternm calls.  The secret key of cz_box_keypair comes from the OS
 * CSPRNG (getrandom), the public key from X25519(sk, 9) on the device. */
int cz_scalarmult(uint8_t q[32], const uint8_t n[32], const uint8_t p[32]);             /* crypto_scalarmult */
int cz_box_keypair(uint8_t pk[32], uint8_t sk[32]);                                      /* Curve.java:100-115 */
int cz_box_beforenm(uint8_t k[32], const uint8_t pk[32], const uint8_t sk[32]);          /* Curve.java:124-127 */
int cz_box(uint8_t *c, const uint8_t *m, uint64_t mlen, const uint8_t n[24], const uint8_t pk[32],
           const uint8_t sk[32]);                                                        /* Curve.java:183-193 */
int cz_box_open(uint8_t *m, const uint8_t *c, uint64_t clen, const uint8_t n[24], const uint8_t pk[32],
                const uint8_t sk[32]);                                                   /* Curve.java:149-157 */
/* Device batches for connection churn (one lane per key agreement, 32-byte records):
 * out[i] = X25519(scalars[i], points[i]) (points NULL = base point 9);
 * k[i] = beforenm(pk[i], sk[i]) = HSalsa20(X25519(sk[i], pk[i]), 0^16). */
int cz_x25519_batch(const void *d_scalars, const void *d_points, void *d_out, uint32_t count, void *stream);
int cz_beforenm_batch(const void *d_pk, const void *d_sk, void *d_k, uint32_t count, void *stream);

/* ---- 10. CURVE handshake: HELLO / WELCOME / INITIATE / READY (+ ERROR) -----------------------------
 * The state machines of CurveClientMechanism (:80-124, :246-429) and CurveServerMechanism
 * (:77-126, :227-517) with every box / open / secretbox / beforenm / X25519 on the GPU (section 9).
 * A handshake object is created in the reference constructor's state (fresh short-term key pair,
 * cnNonce = cnPeerNonce = 1); the caller moves ZMTP command bodies between the peers:
 *   cz_hs_next_command   = Mechanism.nextHandshakeCommand: CZ_OK with a command to send,
 *                          CZ_EAGAIN when there is nothing to send in this state;
 *   cz_hs_process_command = Mechanism.processHandshakeCommand: CZ_OK, or CZ_EPROTO with
 *                          cz_hs_event() = the ZMQ_PROTOCOL_ERROR_* event the reference raises,
 *                          CZ_EINVAL for an incompatible peer Socket-Type (parseMetadata);
 *   cz_hs_status         = Mechanism.status: CZ_HS_HANDSHAKING / READY / ERROR.
 * Once READY, cz_hs_session yields cnPrecom and the nonce counters that cz_mech_create /
 * cz_engine_add_conn take; cz_hs_mechanism / cz_engine_add_session do both steps.
 * socket_type: ZMQ_PAIR = 0 ... ZMQ_GATHER = 20 (zmq/ZMQ.java:50-70); the Socket-Type property and,
 * for REQ / DEALER / ROUTER, the Identity property are sent in INITIATE / READY.
 * ephemeral_secret / entropy (tests only, NULL in production): a fixed short-term secret and the
 * bytes the reference's Curve.random() draws return, in order (client: the 16-byte vouch nonce;
 * server: cookie nonce 16, cookie key 32, WELCOME nonce 16).  ZAP (out of scope): with
 * cz_hs_set_zap(hs, 1) the server waits after INITIATE for cz_hs_zap_reply(hs, "200" | "4xx" ...). */
typedef struct cz_hs cz_hs;
#define CZ_HS_HANDSHAKING 0
#define CZ_HS_READY 1
#define CZ_HS_ERROR 2
int cz_hs_create(cz_hs **hs, int as_server, const uint8_t public_key[32], const uint8_t secret_key[32],
                 const uint8_t server_key[32], int socket_type, const uint8_t *identity, uint32_t identity_len,
                 const uint8_t *ephemeral_secret, const uint8_t *entropy, uint32_t entropy_len);
void cz_hs_destroy(cz_hs *hs);
int cz_hs_next_command(cz_hs *hs, uint8_t *out, uint32_t cap, uint32_t *len);
int cz_hs_process_command(cz_hs *hs, const uint8_t *cmd, uint64_t size);
int cz_hs_status(const cz_hs *hs);
int cz_hs_event(const cz_hs *hs);
/* client: the status code (300..500) of a well-formed ERROR from the server, else 0 */
int cz_hs_error_status(const cz_hs *hs);
int cz_hs_set_zap(cz_hs *hs, int on);
int cz_hs_zap_reply(cz_hs *hs, const char *status_code);
/* server, after INITIATE: the client's long-term public key C (what a ZAP request carries) */
int cz_hs_client_key(const cz_hs *hs, uint8_t key[32]);
int cz_hs_session(const cz_hs *hs, uint8_t precom[32], uint64_t *cn_nonce, uint64_t *cn_peer_nonce);
/* a property of the peer's metadata (INITIATE / READY), e.g. "Socket-Type", "Identity" */
int cz_hs_peer_property(const cz_hs *hs, const char *name, const uint8_t **value, uint32_t *len);
cz_mech *cz_hs_mechanism(const cz_hs *hs, int device);
int cz_engine_add_session(cz_engine *e, const cz_hs *hs);
/* host only: Metadata.read + parseMetadata's Socket-Type check (CZ_OK / CZ_EPROTO / CZ_EINVAL), and the
 * metadata block a socket of this type sends (returns its size; written when it fits in cap) */
int cz_zmtp_metadata_check(const uint8_t *buf, uint64_t len, int socket_type);
uint32_t cz_zmtp_metadata(int socket_type, const uint8_t *identity, uint32_t identity_len, uint8_t *out, uint32_t cap);

/* ---- 11. batched server handshake: N HELLO -> N WELCOME, N INITIATE -> N READY ---------------------
 * The server half of the CURVE handshake (CurveServerMechanism.java:254-517: processHello :254-299,
 * produceWelcome :301-358, processInitiate :360-471, produceReady :473-507, produceError :509-517) for
 * many connections per call: a reconnect storm in front of a ROUTER / XPUB is accepted in two device
 * stages whose launch count does not depend on the number of connections, and ends in sessions
 * cz_engine takes.  Each item behaves as one cz_hs server object (section 10, no ZAP handler) fed the
 * same command, with two differences: a slot that has seen an INITIATE, accepted or not, takes no
 * second one (CZ_EINVAL), and a failed slot stays allocated until cz_acceptor_release.
 * Not thread-safe: one acceptor per IO thread, as cz_engine.  No device: cz_acceptor_create returns
 * CZ_EHIP.  ZAP is out of scope: apply an allow-list with cz_acceptor_client_key before sending READY. */
typedef struct cz_acceptor cz_acceptor;
typedef struct cz_accept_result { /* one per command of a batch */
    int32_t rc;         /* CZ_OK, CZ_EPROTO, CZ_EINVAL (bad slot / incompatible Socket-Type), CZ_EAGAIN (table full) */
    int32_t event;      /* the ZMQ_PROTOCOL_ERROR_* event cz_hs would report, else 0 */
    int32_t slot;       /* pending-connection handle (>= 0) or -1 */
    uint32_t reply_len; /* bytes written to this command's reply slot (0 = nothing to send) */
} cz_accept_result;
/* CurveServerMechanism's constructor :55-75 for max_pending connections in flight; socket_type and
 * identity as cz_hs_create (the READY metadata) */
int cz_acceptor_create(cz_acceptor **a, const uint8_t secret_key[32], int socket_type, const uint8_t *identity,
                       uint32_t identity_len, uint32_t max_pending, int device);
void cz_acceptor_destroy(cz_acceptor *a);
/* Stage 1, processHello + produceWelcome / produceError (:254-358, :509-517).  cmds: count command
 * bodies at off[i], size[i], all inside [0, cmds_bytes); reply: count slots of reply_stride (>= 168)
 * bytes.  Per item: a wrong name -> CZ_EPROTO / CZ_ZMTP_UNEXPECTED_COMMAND, a size other than 200 or a
 * version other than 1.0 -> CZ_EPROTO / CZ_ZMTP_MALFORMED_COMMAND_HELLO (no reply, no slot); a box that
 * does not open -> CZ_OK with event CZ_ZMTP_CRYPTOGRAPHIC, the 7-byte ERROR command as reply, no slot;
 * a good HELLO -> the 168-byte WELCOME and a slot; CZ_EAGAIN when max_pending slots are in use.
 * test_secrets (count x 32) / test_entropy (count x 64: cookie nonce 16, cookie key 32, WELCOME nonce
 * 16 -- cz_hs_create's order): NULL in production (getrandom).  Bad arguments (null pointers, a command
 * outside cmds_bytes, a short stride): CZ_EINVAL for the call, nothing written. */
int cz_acceptor_hello(cz_acceptor *a, uint32_t count, const uint8_t *cmds, uint64_t cmds_bytes, const uint64_t *off,
                      const uint32_t *size, uint8_t *reply, uint64_t reply_stride, cz_accept_result *res,
                      const uint8_t *test_secrets, const uint8_t *test_entropy);
/* Stage 2, processInitiate + produceReady (:360-507) for pending slots (slot[i] from stage 1);
 * reply_stride >= 288.  Per item: events as cz_hs (CZ_ZMTP_MALFORMED_COMMAND_INITIATE for a size below
 * 257 or a box over 16 + 144 + 256, CZ_ZMTP_CRYPTOGRAPHIC for a cookie, INITIATE box or vouch that does
 * not open or a cookie of another connection, CZ_ZMTP_KEY_EXCHANGE for a vouch naming another C'),
 * CZ_EPROTO / CZ_EINVAL from the metadata (Metadata.read, the Socket-Type check), else the READY
 * command (nonce 1).  CZ_EINVAL for a slot that is not waiting for its INITIATE. */
int cz_acceptor_initiate(cz_acceptor *a, uint32_t count, const int32_t *slot, const uint8_t *cmds, uint64_t cmds_bytes,
                         const uint64_t *off, const uint32_t *size, uint8_t *reply, uint64_t reply_stride,
                         cz_accept_result *res);
/* after a CZ_OK stage 2: the same facts cz_hs_session / cz_hs_client_key / cz_hs_peer_property give */
int cz_acceptor_session(const cz_acceptor *a, int32_t slot, uint8_t precom[32], uint64_t *cn_nonce,
                        uint64_t *cn_peer_nonce);
int cz_acceptor_client_key(const cz_acceptor *a, int32_t slot, uint8_t key[32]);
int cz_acceptor_peer_property(const cz_acceptor *a, int32_t slot, const char *name, const uint8_t **value,
                              uint32_t *len);
/* as cz_engine_add_session: returns the connection id */
int cz_engine_add_accepted(cz_engine *e, const cz_acceptor *a, int32_t slot);
/* wipe the slot's secrets (host and device) and free it for reuse */
int cz_acceptor_release(cz_acceptor *a, int32_t slot);
/* slots in use (handed out by stage 1 and not yet released) */
uint32_t cz_acceptor_pending(const cz_acceptor *a);

/* ---- 12. batched client handshake: N HELLO, N WELCOME -> N INITIATE, N READY -> N sessions ----------
 * The client half of the CURVE handshake (CurveClientMechanism.java:246-429: produceHello :246-279,
 * processWelcome :281-316, produceInitiate :318-385, processReady :387-419, processError :421-429) for
 * many connections per call: a process that dials many peers (a collector in front of thousands of
 * publishers, a broker's back end after a restart, a mesh node) connects in three device stages whose
 * launch count does not depend on the number of connections, and ends in sessions cz_engine takes.
 * Each item behaves as one cz_hs client object (section 10) fed the same command -- WELCOME is accepted
 * only by a slot waiting for it and READY only by a slot waiting for that, as there -- with two
 * differences: a slot whose WELCOME or READY was rejected, or that received an ERROR, takes no further
 * command (CZ_EINVAL), and a failed slot stays allocated until cz_connector_release.  A slot named twice
 * in one call: the first item takes it, the second gets CZ_EINVAL.
 * Conventions as section 11: bad arguments (null pointers, a command outside cmds_bytes, a short
 * stride) give CZ_EINVAL for the call with nothing written; results are cz_accept_result records.  Not
 * thread-safe: one connector per IO thread.  No device: cz_connector_create returns CZ_EHIP. */
typedef struct cz_connector cz_connector;
/* CurveClientMechanism's constructor :55-78 for max_pending connections in flight.  public_key /
 * secret_key: the client's long-term pair; socket_type and identity as cz_hs_create (the INITIATE
 * metadata: more than 256 bytes of it is CZ_EMSGSIZE here, where cz_hs fails at INITIATE time). */
int cz_connector_create(cz_connector **c, const uint8_t public_key[32], const uint8_t secret_key[32], int socket_type,
                        const uint8_t *identity, uint32_t identity_len, uint32_t max_pending, int device);
void cz_connector_destroy(cz_connector *c);
/* Stage 1, the constructor's short-term key pair :66 and produceHello :246-279.  server_keys: count x
 * 32 bytes, one server key per connection (a batch may dial different servers); reply: count slots of
 * reply_stride (>= 200) bytes.  Per item: the 200-byte HELLO (nonce 1) and a slot, or CZ_EAGAIN when
 * max_pending slots are in use.  test_secrets (count x 32 short-term secrets): NULL in production
 * (getrandom). */
int cz_connector_hello(cz_connector *c, uint32_t count, const uint8_t *server_keys, uint8_t *reply, uint64_t reply_stride,
                       cz_accept_result *res, const uint8_t *test_secrets);
/* Stage 2, processWelcome + produceInitiate (:281-385) for slots that wait for their WELCOME (slot[i]
 * from stage 1).  cmds: count command bodies at off[i], size[i], all inside [0, cmds_bytes); reply:
 * count slots of reply_stride (>= 513) bytes.  Per item, as cz_hs: another command's name ->
 * CZ_EPROTO / CZ_ZMTP_UNEXPECTED_COMMAND; a size other than 168 -> CZ_ZMTP_MALFORMED_COMMAND_READY
 * (sic); a box that does not open -> CZ_ZMTP_CRYPTOGRAPHIC; an ERROR command -> processError's result
 * (CZ_OK with no reply for a well-formed one, its status code in cz_connector_error_status; else
 * CZ_EPROTO / CZ_ZMTP_MALFORMED_COMMAND_ERROR or CZ_ZAP_MALFORMED_REPLY); else the INITIATE command
 * (nonce 2, 257 + metadata bytes).  CZ_EINVAL for a slot that is not waiting for a WELCOME.
 * test_entropy (count x 16: each item's vouch nonce): NULL in production (getrandom). */
int cz_connector_welcome(cz_connector *c, uint32_t count, const int32_t *slot, const uint8_t *cmds, uint64_t cmds_bytes,
                         const uint64_t *off, const uint32_t *size, uint8_t *reply, uint64_t reply_stride,
                         cz_accept_result *res, const uint8_t *test_entropy);
/* Stage 3, processReady (:387-419) for slots that wait for their READY.  Per item, as cz_hs: a size
 * below 30 or a box over 16 + 16 + 256 -> CZ_ZMTP_MALFORMED_COMMAND_READY; a box that does not open ->
 * CZ_ZMTP_CRYPTOGRAPHIC; CZ_EPROTO / CZ_EINVAL from the metadata (Metadata.read, the Socket-Type
 * check); an ERROR command as in stage 2; else CZ_OK and the slot holds a session.  reply_len is 0. */
int cz_connector_ready(cz_connector *c, uint32_t count, const int32_t *slot, const uint8_t *cmds, uint64_t cmds_bytes,
                       const uint64_t *off, const uint32_t *size, cz_accept_result *res);
/* after a CZ_OK stage 3: the same facts cz_hs_session / cz_hs_peer_property give a client (cn_nonce 3,
 * the READY's nonce as cn_peer_nonce) */
int cz_connector_session(const cz_connector *c, int32_t slot, uint8_t precom[32], uint64_t *cn_nonce,
                         uint64_t *cn_peer_nonce);
int cz_connector_peer_property(const cz_connector *c, int32_t slot, const char *name, const uint8_t **value,
                               uint32_t *len);
/* cz_hs_error_status for a slot: the status code (300..500) of a well-formed ERROR it received, else 0 */
int cz_connector_error_status(const cz_connector *c, int32_t slot);
/* the server key a slot in use was dialled with */
int cz_connector_server_key(const cz_connector *c, int32_t slot, uint8_t key[32]);
/* as cz_engine_add_session: returns the connection id */
int cz_engine_add_connected(cz_engine *e, const cz_connector *c, int32_t slot);
/* wipe the slot's secrets (host and device) and free it for reuse */
int cz_connector_release(cz_connector *c, int32_t slot);
/* slots in use (handed out by stage 1 and not yet released) */
uint32_t cz_connector_pending(const cz_connector *c);

/* ---- 13. bulk session hand-over: N finished handshakes into the engine at once (with section 8) ----
 * The last step of a reconnect storm.  The reference attaches one connection at a time: each
 * StreamEngine takes its own mechanism to READY (StreamEngine.java nextHandshakeCommand :886-912,
 * processHandshakeCommand :914-935, mechanismReady :958) and tears it down alone (unplug / error, :334-370, :1116-1131).  Sections
 * 11 and 12 finish N handshakes in a fixed number of launches; these calls move the N sessions into
 * the engine, and out of it and of the handshake's slot table, in a fixed number as well: one subkey
 * table growth at most, one k_session_subkeys launch (one lane per session and direction), one wipe of
 * the staging and one synchronisation, whatever N is.
 * The add calls are drop-in for the loop of single adds: ids[i] is the id (and the subkey slots are those)
 * that the i-th single call would have returned on the same engine -- ids freed by cz_engine_remove_conn
 * first, last freed first, then new ids in order -- and a slot named twice gives two connections.
 * Per item: a slot that is out of range or holds no completed handshake gives ids[i] = CZ_EINVAL,
 * consumes no id, and the other items proceed (the call returns CZ_OK).  For the call: CZ_EINVAL (null
 * pointers) or CZ_EHIP (any HIP error) leave the engine exactly as it was, with every ids[i] negative.
 * count == 0 returns CZ_OK and launches nothing. */
/* cz_engine_add_conn (the mechanism constructors, CurveClientMechanism.java:55-78 /
 * CurveServerMechanism.java:55-75, with the state of a finished handshake) for count sessions from host
 * keys.  as_server: count flags, NULL = all clients; precoms: count x 32 bytes, staged through pinned
 * memory in one copy and wiped there and on the device before the call returns. */
int cz_engine_add_conns(cz_engine *e, uint32_t count, const uint8_t *as_server, const uint8_t *precoms,
                        const uint64_t *cn_nonce, const uint64_t *cn_peer_nonce, int32_t *ids);
/* cz_engine_add_accepted / cz_engine_add_connected for count slots: cnPrecom is read from the
 * handshake's device state, where it lies until the slot is released, and does not pass through the
 * host (a handshake on another device than the engine: its host copy is staged as above).  Nonces as the
 * single calls set them.  The call returns after the engine's synchronisation, so the slots may be
 * released at once. */
int cz_engine_add_accepted_batch(cz_engine *e, const cz_acceptor *a, uint32_t count, const int32_t *slots,
                                 int32_t *ids);
int cz_engine_add_connected_batch(cz_engine *e, const cz_connector *c, uint32_t count, const int32_t *slots,
                                  int32_t *ids);
/* cz_engine_remove_conn (StreamEngine unplug / error, StreamEngine.java:334-370,1116-1131) for a list:
 * rcs[i] = what the i-th single call would return (CZ_EINVAL for an id that is unknown, already
 * removed or named before in the list; the others proceed), the ids are reused in the order the loop
 * would leave them, and the subkeys are wiped by one launch with one synchronisation. */
int cz_engine_remove_conns(cz_engine *e, uint32_t count, const int *conns, int32_t *rcs);
/* cz_acceptor_release / cz_connector_release (the mechanism's destroy(), Mechanism.java:379) for a list,
 * all or nothing: every slot must be in use and none named twice, else CZ_EINVAL with nothing
 * released; the device records are wiped by one launch on the handshake's stream and the slots freed
 * in list order. */
int cz_acceptor_release_batch(cz_acceptor *a, uint32_t count, const int32_t *slots);
int cz_connector_release_batch(cz_connector *c, uint32_t count, const int32_t *slots);

/* ---- 6. misc -------------------------------------------------------------- */
const char *cz_last_error(void);
const char *cz_version(void);
/* 1 if a HIP device is present and the gfx950 code object loaded */
int cz_device_ok(void);
/* Kernel-variant knob for A/B measurement; returns the previous value or CZ_EINVAL.
 *   "pair": 1 = seal kernels read whole 128-byte input lines per two blocks (default), 0 = per block
 *   "un0":  1 = scalar first Salsa round when the high nonce word is wave-uniform (default), 0 = off
 *   "seglines": 1 = line-staged stores in the segment kernels (default), 0 = direct stores
 *   "shift": 1 = byte-shifted line staging for uniform outputs off 128-byte slots (default)
 *   "shift16": 1 = segment outputs that are 16-byte but not 128-byte aligned through the
 *              byte-shifted line emitter (default), 0 = 128-byte groups at each output's base
 *   "open_ina" / "seal_ina": 1 = line paths for bodies / payloads off 16-byte alignment with
 *              dword-aligned loads (default), 0 = lane-wise unaligned paths
 *   "fanout_min": cz_engine_flush_out takes a publish's run of at least this many frames out of the
 *              segment plan, whatever its length; all such runs of a flush group are sealed by one
 *              cz_seal_fanout_runs call (default 2^18, the count at which one lane per subscriber fills
 *              the device at 4 KiB); 0 = every publish stays on the segment path
 *   "fanout_short": ... and so is a run of at least 64 frames (one full wave) whose payload is at most
 *              this many bytes, unless fanout_min is 0; 0 = rule off.  Default 256, the largest measured
 *              length at which the grouped call is not slower than the segment kernels at every
 *              R x N >= 1024 (100 B: 0.0102 against 0.0179 ms for 16 publishes to 1024 subscribers; 256 B:
 *              0.0150 against 0.0198 ms; 1024 B: 0.0395 against 0.0317 ms, so not 1024) and the routed
 *              flush of 256 publishes to 1024 connections is not slower than the segment-plan flush
 *              (100 B: 2.7 against 6.3 ms; 256 B: 3.8 against 5.6 ms); profiles/fanout/fanout_runs.json
 *   "fanout_split": every other run of at least 64 frames whose payload is at least this many bytes leaves the
 *              segment plan for the flush group's one cz_seal_fanout_split call (section 3e), cut at the segment
 *              length the group's segment plan uses, unless fanout_min is 0; 0 = rule off.  Default 4096, the
 *              smallest measured length from which on the split call is not slower than the segment kernels at
 *              every R x N >= 1024 (4 KiB: 0.0570 against 0.0612 ms for 16 publishes to 1024 subscribers; 64 KiB:
 *              0.542 against 0.558 ms; 1 KiB loses one shape, 0.1461 against 0.1460 ms at 2^18 lanes, so not 1024)
 *              and the routed flush of 256 publishes to 1024 connections is not slower than the segment-plan
 *              flush (4 KiB: 25.1 against 28.7 ms; 64 KiB: 305 against 307 ms); profiles/fanout/fanout_split.json
 *   "fanin_short": cz_engine_flush_in takes a run of at least 64 consecutive received frames (one full wave) of
 *              one body size whose payload is at most this many bytes out of the segment plan; all such runs of a
 *              flush group are opened by one cz_open_fanin_runs call (section 3f); 0 = rule off.  Default 100, the
 *              largest measured length at which the fan-in call is not slower than cz_open_segments at every
 *              R x N >= 1024 (100 B: 0.0104 against 0.0122 ms for 16 runs of 1024 bodies; 256 B: 0.0142 against
 *              0.0151 ms; 1024 B: 0.0394 against 0.0304 ms, so not 1024) and the routed flush of 1024 connections x
 *              16 frames is not slower than the unrouted one (100 B: 1.447 against 1.447 ms; 256 B: 1.567 against
 *              1.554 ms, so not 256: such a flush is host- and copy-bound); profiles/fanin/fanin.json
 *   "fanin_split": every other such run of at least 64 received frames whose payload is at least this many bytes leaves
 *              the segment plan for the flush group's one cz_open_fanin_split call (section 3g), cut at the flush's
 *              own segment length; fanin_short keeps precedence; 0 = rule off.  Default 0: the rule that set
 *              fanout_split asks the split call to be not slower than cz_open_segments at every R x N >= 1024 at every
 *              measured length from the default up, and the routed flush_in of 1024 connections x 16 and x 256 frames
 *              to be not slower than the unrouted one.  The split call is ahead at 19 of 20 shapes (4 KiB: 0.0585
 *              against 0.0597 ms for 16 runs of 1024 bodies; 16 KiB: 0.1850 against 0.1865 ms) and the routed flush at
 *              all 8 (1 KiB x 16: 2.03 against 3.39 ms; 64 KiB x 256: 368.8 against 370.3 ms), but 64 KiB loses one
 *              shape (16 runs of 1024 bodies: 0.6197 against 0.6033 ms), so no length qualifies.  A caller whose runs
 *              stay below 64 KiB can set 1024; profiles/fanin/fanin_split.json
 *   "scan_in": cz_engine_flush_in parses on the device (section 7b, cz_engine_scan_frames) when at least 64 live
 *              connections have received bytes and each holds at most this many; 0 = off.  Default 0, by the rule that set fanin_short: the largest
 *              measured per-connection byte count at which the scanned flush is not slower than the unscanned one at every
 *              measured shape at or below it.  The smallest shape already loses (1024 connections x 16 frames of 100 B,
 *              2160 bytes each: 1.545 against 1.440 ms; 64 x one 4 KiB frame: 0.307 against 0.186 ms; 16 x 256 B: 1.572
 *              against 1.502 ms): the host parse it removes ran behind the H2D, the totals read-back does not.  It wins
 *              at 16 x 1 KiB (1.822 against 2.825 ms) and 16 x 4 KiB (2.945 against 3.588 ms); a caller whose flushes are
 *              a thousand connections with such frames can set 65536; profiles/scan/scan.json */
int cz_tune(const char *key, int value);

#ifdef __cplusplus
}
#endif
#endif
