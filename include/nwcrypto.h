/*
 * nwcrypto — MI355X-native Ed25519 verification and SHA-512 digesting for Narwhal/Bullshark.
 *
 * C ABI drop-in boundary for the reference ``crypto`` crate's hot path.
 * Every entry point names the reference interface it replaces.  All buffers are caller-owned;
 * calls are synchronous unless the name ends in ``_dev`` (those enqueue on a caller stream and
 * take device pointers).  There is no CPU fallback: with no usable GPU every call returns
 * NW_ERR_DEVICE.
 *
 * Threading (the worker calls verify_batch from 64 rayon threads, worker/src/processor.rs:75-79):
 * a context is reentrant.  Each call leases its own stream and scratch from a pool (up to 64
 * concurrent calls; more wait), so calls from different threads run concurrently on the GPU.  The
 * key cache is read-shared by verify calls; nw_committee_load takes it exclusively and waits for
 * in-flight calls first.  A ``_dev`` call's scratch stays reserved until its work completes on the
 * caller's stream.  nw_last_error() reports the calling thread's last error.
 *
 * Batch coefficients: every batch entry point takes ``zseed``, which MUST be 32 fresh CSPRNG bytes
 * per call in production (the reference draws z_i from thread_rng on every call).  With a fixed or
 * public seed an attacker can build invalid signatures whose batch terms cancel.  NULL is rejected
 * with NW_ERR_ARG.
 *
 * Verdict semantics are those of ed25519-dalek 1.0.1 (default features + "batch"):
 *   strict  = crypto::Signature::verify      (crypto/src/lib.rs:200-204) -> verify_strict
 *   batch   = crypto::Signature::verify_batch (crypto/src/lib.rs:206-219) -> dalek::verify_batch,
 *             with the random 128-bit coefficients drawn from a seeded ChaCha20 stream
 *             (NW-Z v1, see nw_chacha.h) instead of thread_rng.
 */
#ifndef NWCRYPTO_H
#define NWCRYPTO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Status codes.  NW_ERR_SIG is the reference's opaque ``ed25519::Error`` (CryptoError,
 * crypto/src/lib.rs:18) that callers map to DagError::InvalidSignature (primary/src/error.rs:27-28). */
#define NW_OK 0
#define NW_ERR_SIG 1
#define NW_ERR_ARG 2
#define NW_ERR_DEVICE 3
#define NW_ERR_NOMEM 4

/* ABI revision of this header.  2: nw_verify_certs_dev gained ``d_status`` before ``stream`` and
 * every batch entry point rejects a NULL zseed (revision 1 = nwcrypto 0.1).  The shared library's
 * soname carries it (libnwcrypto.so.2), so a caller built against revision 1 does not load this
 * library by accident; callers may also compare nw_abi_version() with NW_ABI_VERSION at startup. */
#define NW_ABI_VERSION 2

/* Per-signature flag bits written by the verify kernels (nw_verify_certs sig_flags output). */
#define NW_F_S_OK 0x001u      /* S < l (ed25519 high-bit check + dalek check_scalar) */
#define NW_F_A_OK 0x002u      /* public key decodes (dalek::PublicKey::from_bytes) */
#define NW_F_MATCH 0x004u     /* R decodes and R == sB - hA (strict equation holds) */
#define NW_F_STRICT 0x008u    /* verify_strict verdict */
#define NW_F_A_SMALL 0x010u   /* A is of small order */
#define NW_F_R_SMALL 0x020u   /* R is of small order (meaningful when MATCH) */
#define NW_F_SLOW 0x1000u     /* needed the exact batch equation (rare path) */
#define NW_F_R_BAD 0x2000u    /* R failed to decode (found on the exact path) */
/* Bits 0x4000 and above (other than the torsion coefficient at 0x700) are reserved: never set in
 * returned flags.  A signature inside no certificate's vote range gets flags 0 (no verdict). */

/* Opaque extended-point encoding exchanged between shards of one split batch
 * (nw_verify_batch_partial / nw_points_sum_is_identity): 160 bytes. */
#define NW_POINT_BYTES 160

typedef struct nw_ctx nw_ctx;

/* nw_opts.flags */
#define NW_OPT_NO_KEY_NEGTAB 0x1u     /* never store the key tables' negated copies (half the HBM per key;
                                         k_verify's key pass then negates entries in the addition) */

typedef struct nw_opts {
    int device;        /* HIP device ordinal (one process per GPU; -1 = current device) */
    uint32_t flags;    /* NW_OPT_* bits below; other bits are reserved (NW_ERR_ARG) */
    size_t max_keys;   /* key-cache capacity in keys.  0 = as many as the key budget holds.  The key
                          budget is the HBM free on the device at the first nw_committee_load (after
                          this context's basepoint table and anything other contexts or processes
                          hold) less a workspace reserve of max(16 GiB, 1/16 of HBM): ~258 GB on an
                          otherwise idle MI355X.  In committee mode (key_window -1) a non-zero
                          max_keys declares every key the context will ever load: the window is sized
                          for max_keys keys and the first load allocates all of them at once (the
                          worker's two Processors: max_keys = 200,000, two loads of 100,000). */
    int key_window;    /* key comb window: 8, 9, 12, 13, 16 or 20 bits.  0 = auto at the first load (16
                          for <= 384 keys, 12 for <= 12288 keys, else 8); -1 = committee mode: the
                          widest window whose tables fit the key budget is used, for max_keys keys
                          when set, else for the first load's keys with 25% headroom (on an idle
                          MI355X: W20 up to ~236 keys, W16 up to ~3,000, W13 up to ~19,600: a
                          10,000-validator committee; W9 up to ~216,000: the worker's 100,000 keys,
                          or its 200,000 declared through max_keys).  Table bytes per key: w8 0.53 MB,
                          w9 0.95 MB, w12 5.77 MB, w13 10.5 MB, w16 67.1 MB, w20 872 MB; additions per
                          signature 32 / 29 / 22 / 20 / 16 / 13; twice the bytes when the tables
                          carry their negated copies (nw_key_negtab).  (The basepoint comb is fixed
                          at w24: 11 additions, 11.8 GB, shared by every context of the process on
                          the same device.) */
} nw_opts;

/* One certificate: its votes are sig[first_vote .. first_vote + n_votes). */
typedef struct nw_cert {
    uint32_t first_vote;
    uint32_t n_votes;
} nw_cert;

/* ---- context ------------------------------------------------------------------------------- */
int nw_ctx_create(nw_ctx** out, const nw_opts* opts);
void nw_ctx_destroy(nw_ctx* ctx);
/* Human-readable description of the calling thread's last error. */
const char* nw_last_error(const nw_ctx* ctx);

/* ---- committee / key cache -------------------------------------------------------------------
 * Replaces the per-vote ``dalek::PublicKey::from_bytes`` decompression at crypto/src/lib.rs:216
 * (and :202) with a one-time decompression + fixed-base table build per key.  A key that fails
 * to decode is still cached with its failure recorded, so verification returns NW_ERR_SIG for it
 * exactly where the reference's ``?`` would.  Returns the slot index of each key in ``slot_out``
 * (may be NULL).  Keys already cached keep their slot. ``stake`` may be NULL (stake 0). */
int nw_committee_load(nw_ctx* ctx, const uint8_t (*pk)[32], const uint32_t* stake, size_t n,
                      uint32_t* slot_out);
/* Number of cached keys. */
size_t nw_committee_size(const nw_ctx* ctx);
/* Key comb window in use (8 / 12 / 16 / 20; 0 before the first load, or -1 while committee mode
 * has not sized it yet). */
int nw_key_window(const nw_ctx* ctx);
/* 1 when every cached key table is stored with its negated copy (decided at the first load: when
 * twice the tables fit the HBM budget of a committee-mode, declared-size (nw_opts.max_keys) or
 * explicit-window context; never with an automatic window; the flag NW_OPT_NO_KEY_NEGTAB in
 * nw_opts.flags disables it), else 0.  Verdicts are the
 * same either way; only k_verify's key pass differs (no conditional negation with the copies). */
int nw_key_negtab(const nw_ctx* ctx);
/* Basepoint comb window this library was built with (additions per s*B = ceil(256 / w)). */
int nw_base_window(void);

/* ---- verification ----------------------------------------------------------------------------
 * Keys: nw_verify_strict[_many] and nw_verify_batch accept ANY key, like the reference (which
 * decompresses every key per call, crypto/src/lib.rs:202,216).  When every key of a call is in the
 * key cache the call uses the cached comb tables; otherwise it runs the variable-base path (strict:
 * per-signature decompression + windowed scalar multiplication; batch: a Pippenger multi-scalar
 * multiplication) and leaves the cache unchanged.  Verdicts are identical on both paths.
 *
 * crypto::Signature::verify (crypto/src/lib.rs:200-204): strict single verify of ``msg``. */
int nw_verify_strict(nw_ctx* ctx, const uint8_t* msg, size_t len, const uint8_t pk[32],
                     const uint8_t sig[64]);

/* Bulk strict verify (Header::verify / Vote::verify callers, primary/src/messages.rs:48-67,131-142):
 * n independent (msg_i, pk_i, sig_i); ok[i] = 1 when verify_strict accepts. */
int nw_verify_strict_many(nw_ctx* ctx, const uint8_t* const* msg, const size_t* len,
                          const uint8_t (*pk)[32], const uint8_t (*sig)[64], size_t n, uint8_t* ok);

/* dalek::verify_batch as called by crypto::Signature::verify_batch (crypto/src/lib.rs:218) and by
 * the worker's simulated load (worker/src/processor.rs:78): one verdict for n signatures over
 * per-signature messages.  Coefficients: NW-Z v1 stream ``zseed`` with batch index ``batch_index``.
 * Returns NW_OK / NW_ERR_SIG. */
int nw_verify_batch(nw_ctx* ctx, const uint8_t* const* msg, const size_t* len,
                    const uint8_t (*pk)[32], const uint8_t (*sig)[64], size_t n,
                    const uint8_t zseed[32], uint64_t batch_index);

/* Many dalek::verify_batch calls over arbitrary keys in one submission (the worker's direct call,
 * worker/src/processor.rs:78, without a key cache): batch b is the next counts[b] signatures;
 * batch_ok[b] = 1 iff its batch equation holds (coefficients: NW-Z v1 with batch index
 * batch_base + b).  Always the variable-base Pippenger path. */
int nw_verify_batches_pk(nw_ctx* ctx, size_t nb, const uint32_t* counts, const uint8_t* const* msg,
                         const size_t* len, const uint8_t (*pk)[32], const uint8_t (*sig)[64],
                         const uint8_t zseed[32], uint64_t batch_base, uint8_t* batch_ok);

/* One shard of a batch split across GPUs: the shard's share of the batch
 * equation, sum z_i R_i + sum (z_i h_i mod l) A_i - (sum z_i s_i mod l) B over its n signatures,
 * with z_i drawn at coefficient index z_offset + i of batch ``batch_index``.  ``point`` receives the
 * sum (NW_POINT_BYTES, opaque); *bad = 1 when a signature fails to parse or decode (the batch is
 * then Err).  The batch verdict is Ok iff no shard is bad and nw_points_sum_is_identity of all
 * shards' points is true. */
int nw_verify_batch_partial(nw_ctx* ctx, const uint8_t* const* msg, const size_t* len,
                            const uint8_t (*pk)[32], const uint8_t (*sig)[64], size_t n,
                            const uint8_t zseed[32], uint64_t batch_index, uint32_t z_offset,
                            uint8_t point[NW_POINT_BYTES], int* bad);
int nw_points_sum_is_identity(nw_ctx* ctx, const uint8_t (*points)[NW_POINT_BYTES], size_t k,
                              int* is_identity);

/* Certificate bulk path (Certificate::verify's batch step, primary/src/messages.rs:214, for many
 * certificates at once).  Signers are committee slots (nw_committee_load).  msg[c] is the 32-byte
 * certificate digest.  Vote ranges must be pairwise disjoint (a vote's coefficient and exact-path
 * term belong to one certificate): overlapping ranges are NW_ERR_ARG; a signature inside no range
 * gets sig_ok 0 and affects no certificate.  Outputs (each may be NULL):
 *   cert_ok[c]        1 iff Signature::verify_batch(msg[c], votes of c) is Ok
 *   sig_ok[v]         1 iff verify_strict accepts vote v (the per-signature fallback bitmap)
 *   accepted_stake[c] sum of signer stake over votes with sig_ok = 1
 * Coefficients for certificate c use batch index cert_base + c. */
int nw_verify_certs(nw_ctx* ctx, const nw_cert* certs, size_t ncerts, const uint8_t (*sig)[64],
                    const uint32_t* signer_slot, const uint8_t (*msg)[32], const uint8_t zseed[32],
                    uint64_t cert_base, uint8_t* cert_ok, uint8_t* sig_ok, uint64_t* accepted_stake);

/* Many independent dalek::verify_batch calls in one submission — the worker's simulated
 * transaction-signature load (worker/src/processor.rs:75-79: 64 chunks per batch, 8-byte messages,
 * keys fixed at spawn).  Batch b covers signatures [first[b], first[b] + n[b]); signature i signs
 * msg[i] (len[i] bytes) under key-cache slot signer_slot[i] (nw_committee_load).  Outputs (each
 * may be NULL): batch_ok[b] = 1 iff verify_batch of batch b is Ok (coefficients: NW-Z v1 with
 * batch index batch_base + b); sig_ok[i] = verify_strict verdict of signature i. */
int nw_verify_batches(nw_ctx* ctx, size_t nb, const uint32_t* first, const uint32_t* n,
                      const uint8_t* const* msg, const size_t* len, const uint32_t* signer_slot,
                      const uint8_t (*sig)[64], const uint8_t zseed[32], uint64_t batch_base, uint8_t* batch_ok,
                      uint8_t* sig_ok);

/* Device-resident variant for streaming use (inputs already in HBM).  All pointers are device
 * pointers; ``stream`` is a hipStream_t (NULL = default stream).  ``sig_flags`` (uint32 per vote,
 * NW_F_* bits) may be NULL.  The inputs are checked on the device (every vote range inside
 * [0, nsigs), no vote inside two ranges, every signer slot inside the key cache); the kernels clamp
 * them, so bad inputs never fault — their signatures and certificates are rejected.
 *   d_status == NULL: the check is synchronous — the call waits for it on ``stream`` and returns
 *                     NW_ERR_ARG (enqueueing nothing else) when it fails; otherwise it enqueues the
 *                     verification and returns.
 *   d_status != NULL: fully asynchronous — *d_status (device uint32) receives NW_OK or NW_ERR_ARG
 *                     in stream order. */
int nw_verify_certs_dev(nw_ctx* ctx, size_t ncerts, const uint32_t* d_cert_first,
                        const uint32_t* d_cert_nvotes, size_t nsigs, const uint8_t* d_sig64,
                        const uint32_t* d_signer_slot, const uint8_t* d_msg32,
                        const uint8_t zseed[32], uint64_t cert_base, uint8_t* d_cert_ok,
                        uint32_t* d_sig_flags, uint64_t* d_accepted_stake, uint32_t* d_status,
                        void* stream);

/* ---- digests ---------------------------------------------------------------------------------
 * sha2 0.9 Sha512 via ed25519_dalek::Sha512 (primary/src/messages.rs:72-82,147-151,228-232;
 * worker/src/processor.rs:65; worker/src/batch_maker.rs:125).  Callers truncate to 32 bytes. */
int nw_sha512(nw_ctx* ctx, const uint8_t* data, size_t len, uint8_t out[64]);
int nw_sha512_many(nw_ctx* ctx, const uint8_t* base, const uint64_t* off, const uint64_t* len,
                   size_t n, uint8_t (*out)[64]);
/* Device-resident bulk digest: d_base/d_off/d_len/d_out are device pointers.  Each message is one
 * sequential compression chain: a lone 508,052-B worker batch takes ~12-15 ms whatever the number
 * of batches in the call (up to ~1,000 chains run concurrently at that rate), DESIGN.md §5.5. */
int nw_sha512_many_dev(nw_ctx* ctx, const uint8_t* d_base, const uint64_t* d_off,
                       const uint64_t* d_len, size_t n, uint8_t* d_out64, void* stream);

/* Asynchronous many-message digest from host buffers, for a caller that keeps receiving work while
 * the GPU hashes (the worker's Processor loop, worker/src/processor.rs:63-97, replacing one
 * serial Sha512::digest per batch at :65 by one submission per window of batches).  Message i is
 * msg[i] (len[i] bytes); the buffers must stay valid until nw_job_wait returns (the worker keeps
 * each batch until it is stored under its digest anyway).  The call enqueues the upload, the
 * digest kernel and the download and returns a job at once.
 *   nw_job_done(job): 1 when the digests are ready, 0 while in flight, < 0 on a device error.
 *   nw_job_wait(job): blocks until out (n x 64 bytes) holds the digests, then frees the job; every
 *                     job must be waited for exactly once, before nw_ctx_destroy.
 * A job holds one of the context's 64 call workspaces until it is waited for; at most 32 jobs may be
 * unwaited at once (the rest of the pool stays for synchronous calls): a 33rd submit returns
 * NW_ERR_NOMEM at once rather than blocking.  nw_job_done and nw_job_wait serve the Core jobs of
 * nw_core_batch_verify_async as well (nw_job_wait then fills n x 4 verdict bytes) and the worker
 * windows of nw_worker_window_async (n x 88 bytes), and the limit of 32 counts the jobs of all kinds
 * together; so do the signing jobs of nw_sign_digests_async (n x 64) and nw_votes_make_async (n x 212). */
typedef struct nw_job nw_job;
int nw_sha512_many_async(nw_ctx* ctx, const uint8_t* const* msg, const size_t* len, size_t n,
                         uint8_t (*out)[64], nw_job** job);
int nw_job_done(nw_job* job);
int nw_job_wait(nw_job* job);

/* ---- signing (crypto::Signature::new / generate_keypair, crypto/src/lib.rs:163-191) -------------
 * Low-volume in the reference; here it makes synthetic workloads.  RFC 8032 Ed25519 over
 * messages of exactly ``msg_len`` bytes (8 or 32). pk or sig may be NULL. */
int nw_sign_many(nw_ctx* ctx, const uint8_t (*seed)[32], const uint8_t* msgs, size_t msg_len,
                 size_t n, uint8_t (*pk)[32], uint8_t (*sig)[64]);
int nw_sign_many_dev(nw_ctx* ctx, const uint8_t* d_seed32, const uint8_t* d_msgs, size_t msg_len,
                     size_t n, uint8_t* d_pk32, uint8_t* d_sig64, void* stream);

/* ---- signing with a resident key: batched signatures and Vote frames out ------------------------
 * The reply half of Core: for every header it accepts, Core::process_header answers with a vote
 * (primary/src/core.rs:184-206): Vote::new (primary/src/messages.rs:113-129: one SHA-512 of 72 bytes
 * and one Signature::new through the SignatureService, crypto/src/lib.rs:229-249), then
 * bincode::serialize(&PrimaryMessage::Vote(..)).  A signer holds ONE key on the device; a call signs
 * n messages with it in one submission (one upload, one kernel, one download).  nw_sign_many above
 * takes a seed per signature and re-derives the key in every lane; it stays as it is.
 *
 * nw_signer_create: seed = the first 32 bytes of the reference's 64-byte SecretKey.  One small kernel
 * expands it on the device (the library has no host SHA-512) into a record of a mod l, the 32-byte
 * nonce prefix, the compressed public key A and A's base64 string; the staging bytes that held the
 * seed, pinned and device, are overwritten before the call returns.  nw_signer_public: A.
 * nw_signer_destroy waits for every pending call of the context (as nw_committee_load does before it
 * changes the key cache), zeroes the record on the device, then frees it.  nw_ctx_destroy does the same
 * to the record of every signer still alive; such a signer is then good for nw_signer_public and
 * nw_signer_destroy only (every other call with it is NW_ERR_ARG).  A signer reads the basepoint table under the shared key lock, as nw_sign_many_dev
 * does, and never touches the key cache.
 *
 * Threat model: the key lives in HBM, in the clear, for the life of the signer.  As in nw_sign_many,
 * the basepoint comb's table gathers are indexed by digits of the secret nonce and are not
 * constant-time (the one field inversion per wave is: fixed-iteration divsteps).  The signer is for a
 * GPU the node owns and shares with nobody.
 *
 * nw_sign_digests: SignatureService::request_signature for n 32-byte digests: sig[i] = the RFC 8032
 * signature of digest[i], bit for bit what nw_sign_many gives for (seed, digest[i]).
 * nw_votes_make: core.rs:192 + :204 for n accepted headers.  req[i] = header id (32) || round (u64
 * LE) || header author (32), which is exactly Hash for Vote's preimage (messages.rs:145-153);
 * frame[i] = the 212 bytes of bincode::serialize(&PrimaryMessage::Vote(Vote::new(..))) with the
 * signer as the vote's author:
 *     0 u32 1 | 4 id | 36 round | 44 u64 44 | 52 origin base64 | 96 u64 44 | 104 author base64 |
 *     148 signature part1 | 180 part2
 *
 * The _async forms enqueue the same submission and return a job: nw_job_done polls, nw_job_wait
 * fills sig (n x 64) / frame (n x 212) and frees the job.  digest / req may be freed on return; sig /
 * frame must live until the wait.  The jobs count against the 32 unwaited jobs of a context; an
 * nw_committee_load that changes the key cache, and nw_signer_destroy, wait for them on the device.
 *
 * NW_ERR_ARG: NULL ctx, signer, out or job; a NULL array with n > 0; a signer of another context;
 * n above 2^24.  n == 0 is NW_OK with nothing launched (the job form yields a job that is complete). */
typedef struct nw_signer nw_signer;
int nw_signer_create(nw_ctx* ctx, const uint8_t seed[32], nw_signer** out);
int nw_signer_public(const nw_signer* signer, uint8_t pk[32]);
void nw_signer_destroy(nw_signer* signer);

int nw_sign_digests(nw_ctx* ctx, const nw_signer* signer, const uint8_t (*digest)[32], size_t n, uint8_t (*sig)[64]);
int nw_sign_digests_async(nw_ctx* ctx, const nw_signer* signer, const uint8_t (*digest)[32], size_t n,
                          uint8_t (*sig)[64], nw_job** job);

#define NW_VOTE_REQ_BYTES 72
#define NW_VOTE_FRAME_BYTES 212
int nw_votes_make(nw_ctx* ctx, const nw_signer* signer, const uint8_t (*req)[NW_VOTE_REQ_BYTES], size_t n,
                  uint8_t (*frame)[NW_VOTE_FRAME_BYTES]);
int nw_votes_make_async(nw_ctx* ctx, const nw_signer* signer, const uint8_t (*req)[NW_VOTE_REQ_BYTES], size_t n,
                        uint8_t (*frame)[NW_VOTE_FRAME_BYTES], nw_job** job);

/* ---- measurement --------------------------------------------------------------------------
 * When enabled, HIP events are recorded on the launch stream around every k_verify launch; read
 * back (synchronizing those events) the summed device time and launch count, then reset.  Launches
 * of at most 4,096 signatures run k_verify_split with k_finish's work fused into it (no separate
 * k_finish launch): their samples cover verify + finish, so they are not comparable with large
 * launches' samples (k_verify alone) or with builds before that fusion. */
int nw_profile_enable(nw_ctx* ctx, int on);
int nw_profile_read(nw_ctx* ctx, double* verify_ms_total, uint64_t* verify_launches);
/* Same, plus the signatures covered by those launches (the roofline's work per launch). */
int nw_profile_read_sigs(nw_ctx* ctx, double* verify_ms_total, uint64_t* verify_launches,
                         uint64_t* verify_sigs);

/* ---- primary certificate path -------------------------------------
 * Native ingestion of bincode ``PrimaryMessage`` frames (primary/src/primary.rs:236) and the whole
 * of Certificate::verify (primary/src/messages.rs:189-215, Header::verify :48-67) for many
 * certificates: host checks in C++, all crypto on the GPU in three submissions.  Verdicts are the
 * DagError kinds the reference returns (primary/src/error.rs:24-58), checked in its order. */
#define NW_DAG_PENDING (-1)             /* decode only: needs the GPU checks */
#define NW_DAG_OK 0
#define NW_DAG_INVALID_SIGNATURE 1      /* DagError::InvalidSignature */
#define NW_DAG_SERIALIZATION 2          /* DagError::SerializationError (bincode / base64 key) */
#define NW_DAG_INVALID_HEADER_ID 3      /* DagError::InvalidHeaderId */
#define NW_DAG_MALFORMED_HEADER 4       /* DagError::MalformedHeader */
#define NW_DAG_UNKNOWN_AUTHORITY 5      /* DagError::UnknownAuthority */
#define NW_DAG_AUTHORITY_REUSE 6        /* DagError::AuthorityReuse */
#define NW_DAG_REQUIRES_QUORUM 7        /* DagError::CertificateRequiresQuorum */
#define NW_DAG_NOT_CERTIFICATE 8        /* a valid PrimaryMessage variant other than Certificate */

/* Committee (config/src/lib.rs:161-240): authority i is name[i] with stake[i]; its worker ids are
 * worker_id[worker_first[i] .. worker_first[i + 1]) (worker_first has n + 1 entries; both NULL =
 * no workers, so any header with a payload is MalformedHeader). */
typedef struct nw_committee {
    size_t n;
    const uint8_t (*name)[32];
    const uint32_t* stake;
    const uint32_t* worker_first;
    const uint32_t* worker_id;
} nw_committee;

typedef struct nw_cert_batch nw_cert_batch;

/* Decoded view of one certificate of a batch.  Pointers stay valid until nw_cert_batch_free. */
typedef struct nw_cert_view {
    int32_t status;                  /* NW_DAG_PENDING, or a final verdict found while decoding
                                        (SERIALIZATION, NOT_CERTIFICATE, OK for genesis) */
    int32_t header_error;            /* Header::verify check after the id (UNKNOWN_AUTHORITY /
                                        MALFORMED_HEADER) or NW_DAG_OK */
    int32_t quorum_error;            /* quorum check (AUTHORITY_REUSE / UNKNOWN_AUTHORITY /
                                        REQUIRES_QUORUM) or NW_DAG_OK */
    uint64_t round;
    const uint8_t* author;           /* 32 B */
    const uint8_t* header_id;        /* 32 B */
    const uint8_t* header_sig;       /* 64 B */
    const uint8_t* header_preimage;  /* Hash for Header (primary/src/messages.rs:70-84) */
    size_t header_preimage_len;
    const uint8_t* cert_preimage;    /* 72 B: Hash for Certificate (:226-234) */
    uint32_t first_vote, n_votes;
    const uint8_t* vote_keys;        /* [n_votes][32] */
    const uint8_t* vote_sigs;        /* [n_votes][64] */
} nw_cert_view;

/* Host only (no context, no GPU): decode n frames and run the host-side checks. */
int nw_cert_batch_decode(const nw_committee* committee, const uint8_t* const* frame, const size_t* len,
                         size_t n, nw_cert_batch** out);
size_t nw_cert_batch_size(const nw_cert_batch* batch);
int nw_cert_batch_view(const nw_cert_batch* batch, size_t i, nw_cert_view* out);
void nw_cert_batch_free(nw_cert_batch* batch);
/* The GPU half: header/certificate digests, header signatures, vote batches.  verdict[i] receives
 * the NW_DAG_* verdict of certificate i.  Batch coefficients (NW-Z v1) use batch index cert_base + j
 * for the j-th certificate that reaches the batch step. */
int nw_cert_batch_verify(nw_ctx* ctx, const nw_cert_batch* batch, const uint8_t zseed[32],
                         uint64_t cert_base, int32_t* verdict);
/* decode + verify + free in one call. */
int nw_certificates_verify(nw_ctx* ctx, const nw_committee* committee, const uint8_t* const* frame,
                           const size_t* len, size_t n, const uint8_t zseed[32], uint64_t cert_base,
                           int32_t* verdict);

/* ---- Core message path: mixed batches --------------------------------
 * What the reference's ``Core`` does with each received ``PrimaryMessage`` (primary/src/core.rs:306-346:
 * sanitize_header, sanitize_vote, sanitize_certificate, one message at a time), for many Header, Vote
 * and Certificate frames in arrival order: one NW_DAG_* verdict per frame, every check in the
 * reference's order.  The host half decodes and runs every check that needs no crypto; the GPU half
 * runs all the crypto as ONE stream-ordered submission (one upload, the digest / link / strict /
 * certificate / verdict kernels, one download, one synchronization).
 *   Header       TooOld (gc_round > round, core.rs:307-310); then Header::verify
 *                (primary/src/messages.rs:48-67): id, UnknownAuthority, MalformedHeader, strict signature.
 *   Vote         TooOld (current.round > round, core.rs:321-324); UnexpectedVote (:327-333); then
 *                Vote::verify (messages.rs:131-142): UnknownAuthority, strict signature over the vote digest.
 *   Certificate  TooOld (core.rs:339-342); then Certificate::verify (messages.rs:189-215): genesis is
 *                Ok; the Header steps; AuthorityReuse / UnknownAuthority / CertificateRequiresQuorum;
 *                the batch equation.
 *   An undecodable frame is NW_DAG_SERIALIZATION (no state check applies to it). */
#define NW_DAG_TOO_OLD 9                /* DagError::TooOld */
#define NW_DAG_UNEXPECTED_VOTE 10       /* DagError::UnexpectedVote */
#define NW_DAG_NOT_CORE_MESSAGE 11      /* a well-formed PrimaryMessage variant other than Header, Vote or
                                           Certificate (the reference panics there, core.rs:374) */

/* nw_core_view.kind */
#define NW_CORE_HEADER 0
#define NW_CORE_VOTE 1
#define NW_CORE_CERTIFICATE 2
#define NW_CORE_OTHER 3                 /* undecodable, or not a Core message */

/* The part of Core's mutable state the sanitize_* checks read (core.rs:307,321-333,339): the
 * garbage-collection round and the header this primary is collecting votes for.  Passing NULL for
 * the state skips those checks (TooOld, UnexpectedVote): the caller then applies them when it applies
 * the verdicts, against the state at that moment. */
typedef struct nw_core_state {
    uint64_t gc_round;
    uint8_t id[32];        /* current_header.id */
    uint64_t round;        /* current_header.round */
    uint8_t author[32];    /* current_header.author */
} nw_core_state;

typedef struct nw_core_batch nw_core_batch;

/* Decoded view of one message of a batch.  Pointers stay valid until nw_core_batch_free; those of
 * fields a kind does not have (and every pointer of an undecodable frame) are NULL. */
typedef struct nw_core_view {
    int32_t kind;                    /* NW_CORE_* */
    int32_t status;                  /* NW_DAG_PENDING, or the verdict decided on the host */
    int32_t header_error;            /* Header, Certificate: UNKNOWN_AUTHORITY / MALFORMED_HEADER or NW_DAG_OK */
    int32_t quorum_error;            /* Certificate: AUTHORITY_REUSE / UNKNOWN_AUTHORITY / REQUIRES_QUORUM or OK */
    uint64_t round;
    const uint8_t* author;           /* 32 B: header author; Vote: the voter */
    const uint8_t* id;               /* 32 B: header id; Vote: the id voted for */
    const uint8_t* origin;           /* 32 B: Vote: the header's author; else = author */
    const uint8_t* signature;        /* 64 B: header signature; Vote: the vote's */
    const uint8_t* preimage;         /* digest preimage: Hash for Header (messages.rs:70-84: author ||
                                        round || payload || parents); Vote: Hash for Vote (:145-153, 72 B) */
    size_t preimage_len;
    const uint8_t* cert_preimage;    /* Certificate: 72 B, Hash for Certificate (:226-234) */
    uint32_t first_vote, n_votes;    /* Certificate */
    const uint8_t* vote_keys;        /* [n_votes][32] */
    const uint8_t* vote_sigs;        /* [n_votes][64] */
    /* A certificate whose votes are carried raw (NW_CORE_DEVICE_VOTES): n_votes is the wire count;
     * vote_keys and vote_sigs are NULL (the votes are decoded on the device only); quorum_error is
     * NW_DAG_OK, because the quorum rules are not evaluated on the host. */
} nw_core_view;

/* nw_core_batch_decode_ex / nw_core_messages_verify_ex flags.
 * NW_CORE_DEVICE_VOTES: decode certificate votes on the GPU.  A certificate is taken raw (its vote
 * section goes to the device as wire bytes; a kernel produces the signatures, signer slots and the
 * AuthorityReuse / UnknownAuthority / RequiresQuorum / SerializationError outcome) when it is regular
 * (every vote's key string is 44 characters long and all the votes the count announces lie inside the
 * frame), the committee has at most 16,384 members, and after the header decode and the host checks it
 * is still NW_DAG_PENDING with header_error == NW_DAG_OK.  Every other certificate is decoded on the
 * host as without the flag.  Verdicts are the same with and without the flag; the batch indices are
 * not (see nw_core_batch_verify). */
#define NW_CORE_DEVICE_VOTES 0x1u

/* Host only (no context, no GPU): decode n frames and run every host-side check of core.rs:306-346,
 * messages.rs:48-67, :131-142 and :189-215 (everything but digests and signatures). */
int nw_core_batch_decode(const nw_committee* committee, const nw_core_state* state, const uint8_t* const* frame,
                         const size_t* len, size_t n, nw_core_batch** out);
/* The same with flags (NW_CORE_*; 0: exactly nw_core_batch_decode; an unknown flag is NW_ERR_ARG). */
int nw_core_batch_decode_ex(const nw_committee* committee, const nw_core_state* state, const uint8_t* const* frame,
                            const size_t* len, size_t n, uint32_t flags, nw_core_batch** out);
size_t nw_core_batch_size(const nw_core_batch* batch);
/* Number of certificate votes the batch carries raw (0 without NW_CORE_DEVICE_VOTES). */
size_t nw_core_batch_raw_votes(const nw_core_batch* batch);
int nw_core_batch_view(const nw_core_batch* batch, size_t i, nw_core_view* out);
void nw_core_batch_free(nw_core_batch* batch);
/* The GPU half of core.rs:306-346 (the digests and signatures of messages.rs:48-67, :131-142,
 * :189-215), one submission: verdict[i] receives the NW_DAG_* verdict of message i.  When the host
 * decided every message nothing is launched and no device is needed (ctx may then be NULL).
 * Batch coefficients (NW-Z v1): the certificates that enter the batch step are those still pending
 * after decoding with header_error == quorum_error == NW_DAG_OK; the j-th of them, in arrival order,
 * uses batch index cert_base + j, and *certs_used (may be NULL) receives their number, so the caller
 * advances cert_base by it.  A certificate whose header then fails on the device (id or signature)
 * still uses up its index (unlike nw_cert_batch_verify, which numbers certificates after the header
 * checks).  In a batch decoded with NW_CORE_DEVICE_VOTES the certificates that enter the batch step
 * are those still pending with header_error == NW_DAG_OK, raw or host-decoded (a host-decoded one
 * also needs quorum_error == NW_DAG_OK, as above); the j-th of them in arrival order uses batch index
 * cert_base + j and *certs_used is their number.  So a raw certificate that then fails its quorum
 * rules on the device uses up an index, where a host-decoded certificate with a quorum_error does
 * not.  zseed == NULL is NW_ERR_ARG. */
int nw_core_batch_verify(nw_ctx* ctx, const nw_core_batch* batch, const uint8_t zseed[32], uint64_t cert_base,
                         int32_t* verdict, uint64_t* certs_used);
/* decode + verify + free in one call: what Core::sanitize_* (core.rs:306-346) returns per frame. */
int nw_core_messages_verify(nw_ctx* ctx, const nw_committee* committee, const nw_core_state* state,
                            const uint8_t* const* frame, const size_t* len, size_t n, const uint8_t zseed[32],
                            uint64_t cert_base, int32_t* verdict, uint64_t* certs_used);
int nw_core_messages_verify_ex(nw_ctx* ctx, const nw_committee* committee, const nw_core_state* state,
                               const uint8_t* const* frame, const size_t* len, size_t n, uint32_t flags,
                               const uint8_t zseed[32], uint64_t cert_base, int32_t* verdict, uint64_t* certs_used);

/* Asynchronous form of nw_core_batch_verify, for a Core that keeps receiving while a batch is checked
 * (the reference's Core::run awaits each sanitize_* in its one task, primary/src/core.rs:351-389):
 * the same checks, the same submission and the same batch indices, but the call returns a job once
 * the work is enqueued.  *certs_used is written before it returns, so the next batch can be submitted
 * at cert_base + *certs_used while this one is in flight.  batch and zseed may be freed as soon as it
 * returns; verdict (n x int32) must stay valid until nw_job_wait(job), which fills it and frees the
 * job.  nw_job_done polls.  Every job must be waited for exactly once, before nw_ctx_destroy; Core
 * and digest jobs share the limit of 32 unwaited jobs (a 33rd submit: NW_ERR_NOMEM at once, nothing
 * enqueued).  A batch the host decided completely yields a job that is already complete: verdict is
 * filled on return, ctx may be NULL, and the job still has to be waited for (which only frees it).
 * A job reads the key cache: an nw_committee_load that adds keys or changes a stake while jobs are in
 * flight first waits for them on the device (it needs no nw_job_wait to have been called). */
int nw_core_batch_verify_async(nw_ctx* ctx, const nw_core_batch* batch, const uint8_t zseed[32], uint64_t cert_base,
                               int32_t* verdict, uint64_t* certs_used, nw_job** job);
/* decode (flags as nw_core_batch_decode_ex) + nw_core_batch_verify_async + free in one call; the frames
 * may be freed on return. */
int nw_core_messages_verify_async(nw_ctx* ctx, const nw_committee* committee, const nw_core_state* state,
                                  const uint8_t* const* frame, const size_t* len, size_t n, uint32_t flags,
                                  const uint8_t zseed[32], uint64_t cert_base, int32_t* verdict,
                                  uint64_t* certs_used, nw_job** job);

/* ---- Core apply: the aggregators (host only, no context, no GPU) ---------------------------------
 * The half of ``Core`` that consumes the verdicts (primary/src/core.rs:216-247 process_vote, :285-296
 * process_certificate, :117-120 process_own_header, :399-409 the gc cleanup; VotesAggregator and
 * CertificatesAggregator, primary/src/aggregators.rs:9-45 and :48-83), driven batch by batch.
 *
 * nw_core_agg_apply takes a batch decoded with a NULL state and its checked verdicts (what
 * nw_core_batch_verify or nw_job_wait wrote) and walks the messages in arrival order:
 *   - a frame whose verdict is NW_DAG_SERIALIZATION or NW_DAG_NOT_CORE_MESSAGE keeps it and takes no
 *     further part;
 *   - every other message first meets the state checks of core.rs:307-310, :321-333, :339-342 against
 *     the aggregator's state AT THAT MOMENT (gc_round, the current header); NW_DAG_TOO_OLD /
 *     NW_DAG_UNEXPECTED_VOTE replace the checked verdict;
 *   - an accepted vote (NW_DAG_OK) goes to the votes aggregator of the current header: a repeated
 *     author is NW_DAG_AUTHORITY_REUSE in verdict[i]; otherwise the vote is recorded, and when the
 *     weight reaches the quorum threshold it is reset to 0 (quorum is reached once), an
 *     NW_CORE_EVENT_CERT_ASSEMBLED event lists the recorded votes, and the assembled certificate goes
 *     at once to the certificates aggregator of the current header's round, origin = its author;
 *   - an accepted certificate goes to its round's certificates aggregator: a repeated origin is
 *     ignored; otherwise it is gathered, and at or past the quorum threshold an NW_CORE_EVENT_PARENTS
 *     event lists everything gathered since the last event of that round.  The weight stays (the
 *     reference's reset is commented out, aggregators.rs:79), so every later distinct origin triggers
 *     again.
 * A member without stake counts as unknown (stake 0); of duplicate names the first holds the stake.
 *
 * Events refer to frames, which the caller keeps: (tag, index) = (the tag given to the apply call that
 * saw the frame, its index in that batch).  The library keeps no message bytes beyond 32-byte names.
 *   CERT_ASSEMBLED  refs[first .. first + count): the votes, in the order recorded (possibly from
 *                   earlier batches); round = the current header's.
 *   PARENTS         refs[first .. first + count): the certificates; one assembled from votes is the
 *                   (tag, index) of the vote that completed it, with assembled = 1; round = theirs.
 * Events, and the refs array (nw_core_agg_refs), stay valid until the next nw_core_agg_apply or
 * nw_core_agg_destroy.  Not thread-safe: one aggregator belongs to one Core. */
#define NW_CORE_EVENT_CERT_ASSEMBLED 1
#define NW_CORE_EVENT_PARENTS 2

typedef struct nw_core_agg nw_core_agg;

typedef struct nw_core_ref {
    uint64_t tag;          /* of the batch that carried the frame */
    uint32_t index;        /* of the frame in that batch */
    uint32_t assembled;    /* PARENTS: 1 = the certificate assembled when this vote arrived */
} nw_core_ref;

typedef struct nw_core_event {
    int32_t kind;          /* NW_CORE_EVENT_* */
    uint64_t round;
    uint64_t tag;          /* batch and ... */
    uint32_t at;           /* ... message that triggered the event */
    uint32_t first, count; /* range of nw_core_agg_refs */
} nw_core_event;

/* gc_depth as in Core (core.rs:44).  The state starts as Core's: gc_round 0, a current header of
 * round 0 with an all-zero id and author. */
int nw_core_agg_create(const nw_committee* committee, uint64_t gc_depth, nw_core_agg** out);
void nw_core_agg_destroy(nw_core_agg* agg);
/* process_own_header (core.rs:117-120): the current header, and a fresh votes aggregator. */
int nw_core_agg_set_header(nw_core_agg* agg, const uint8_t id[32], uint64_t round, const uint8_t author[32]);
/* The cleanup of core.rs:399-409: for consensus_round > gc_depth, gc_round = consensus_round -
 * gc_depth and the certificates aggregators of rounds below it are dropped. */
int nw_core_agg_advance_gc(nw_core_agg* agg, uint64_t consensus_round);
int nw_core_agg_state(const nw_core_agg* agg, nw_core_state* out);
/* verdict: in, the checked verdicts; out, the final ones.  *events / *n_events: this call's events in
 * the order they happened (either may be NULL).  NW_ERR_ARG when a verdict is NW_DAG_PENDING. */
int nw_core_agg_apply(nw_core_agg* agg, const nw_core_batch* batch, uint64_t tag, int32_t* verdict,
                      const nw_core_event** events, size_t* n_events);
int nw_core_agg_refs(const nw_core_agg* agg, const nw_core_ref** refs, size_t* n);

/* ---- worker windows (worker/src/processor.rs:63-81) ---------------------------------------------
 * What the reference's Processor does per received batch: the digest (:65) and, with
 * enable_verification, the simulated signature load (:67-81), for a whole window of serialized
 * batches in ONE asynchronous job, against a signature set that stays in HBM from spawn.
 *
 * nw_sigset is Processor::spawn's fixed load (:46-58): n (message, key-cache slot, signature)
 * triples, uploaded once.  nw_sigset_create takes the key lock shared and rejects a slot outside the
 * key cache (NW_ERR_ARG): load the keys first (nw_committee_load); slots stay valid across later
 * loads because cached keys keep their slot.  The set owns its device allocation, outside the call
 * workspaces.  nw_sigset_destroy only after every job that uses the set has been waited for. */
typedef struct nw_sigset nw_sigset;
int nw_sigset_create(nw_ctx* ctx, const uint8_t* const* msg, const size_t* len, const uint32_t* signer_slot,
                     const uint8_t (*sig)[64], size_t n, nw_sigset** out);
size_t nw_sigset_size(const nw_sigset* set);
void nw_sigset_destroy(nw_sigset* set);

#define NW_WORKER_OK 0             /* hashed; every chunk Ok (or nothing to verify) */
#define NW_WORKER_VERIFY_FAILED 1  /* a chunk is Err: the reference's unwrap panics (processor.rs:78) */
#define NW_WORKER_MALFORMED 2      /* bincode::deserialize fails: the reference panics (processor.rs:68) */

typedef struct nw_worker_result {   /* 88 bytes */
    uint8_t digest[64];   /* Sha512::digest(&batch) (:65); the reference keeps [..32]; always filled */
    int64_t n_tx;         /* WorkerMessage::Batch: its transactions; -1: BatchRequest, malformed, or not parsed */
    uint64_t chunk_ok;    /* bit c = verify_batch verdict of chunk c (:75-79); all ones when nothing was verified */
    uint32_t verified;    /* min(set size, n_tx) (:70); 0 when nothing was verified */
    int32_t status;       /* NW_WORKER_* */
} nw_worker_result;

/* Host only, no context, no GPU: what bincode::deserialize::<WorkerMessage> decides about one frame
 * (processor.rs:68-69; worker/src/worker.rs:37-40).  bincode 1.3, fixint, little endian: u32 variant;
 * Batch (0) = u64 count, then each transaction as u64 length + bytes; BatchRequest (1) = u64 count,
 * that many 32-byte digests, then the requestor's key as its base64 string (u64 length + bytes,
 * crypto/src/lib.rs:94-112; at least 32 decoded bytes).  Trailing bytes after a well-formed message
 * are accepted, as bincode::deserialize accepts them.  NW_OK with *n_tx = the transaction count
 * (Batch) or -1 (BatchRequest: ``if let WorkerMessage::Batch`` does not verify it); NW_ERR_ARG for a
 * malformed frame (the reference's unwrap panics) or a NULL argument.  Counts and lengths up to
 * 2^64 - 1 neither wrap a position nor allocate. */
int nw_worker_frame_count(const uint8_t* frame, size_t len, int64_t* n_tx);

/* One window of nb serialized batches, frame[i] (len[i] bytes), as one asynchronous job: one upload,
 * the digests, the verify load and one download of out[nb].  The frames must stay valid until
 * nw_job_wait, as for nw_sha512_many_async; out (nb x sizeof(nw_worker_result)) is filled by
 * nw_job_wait; nw_job_done polls.  The job counts against the limit of 32 unwaited jobs.
 *
 * set == NULL is enable_verification == false: frames are hashed and not parsed; every result is
 * NW_WORKER_OK with n_tx -1, verified 0 and chunk_ok all ones; zseed may be NULL.
 *
 * With a set every frame is parsed on the host by the rule of nw_worker_frame_count.  The j-th
 * VERIFYING frame of the call is the j-th frame, in arrival order, that parsed as a Batch (one with
 * 0 transactions included).  It verifies the set's first count = min(set size, n_tx) signatures
 * (:70) as 64 chunks, chunk c = [count*c/64, min(count, count*(c+1)/64)) (:76-77, in 64-bit), chunk
 * c with NW-Z v1 batch index batch_base + 64 j + c: chunk_ok bit c is what nw_verify_batches returns
 * for those 64 ranges over the same triples with batch_base + 64 j.  An empty chunk is Ok.  A
 * malformed frame (NW_WORKER_MALFORMED, n_tx -1) still gets its digest, because the reference hashes
 * at :65 before it panics at :68; a BatchRequest is NW_WORKER_OK with n_tx -1; neither uses batch
 * indices.  *batches_used (may be NULL) = 64 x (number of verifying frames), written before the
 * call returns, so the next window can be submitted (batch_base + *batches_used) while this one is
 * in flight.  zseed: 32 fresh CSPRNG bytes per call, as for every batch entry point.
 *
 * The job reads the key tables: an nw_committee_load that adds keys while it is in flight waits for
 * it on the device, as for Core jobs.  NW_ERR_ARG: NULL ctx, out or job, NULL zseed with a set, a set
 * of another context, nb or the window's virtual signature total (the sum of count) above 0xFFFFFFF0. */
int nw_worker_window_async(nw_ctx* ctx, const nw_sigset* set, const uint8_t* const* frame, const size_t* len,
                           size_t nb, const uint8_t zseed[32], uint64_t batch_base, nw_worker_result* out,
                           uint64_t* batches_used, nw_job** job);
/* The same, submit + wait: out is filled on return. */
int nw_worker_window(nw_ctx* ctx, const nw_sigset* set, const uint8_t* const* frame, const size_t* len, size_t nb,
                     const uint8_t zseed[32], uint64_t batch_base, nw_worker_result* out, uint64_t* batches_used);

/* Library build identifier (gfx target, build date). */
const char* nw_version(void);
/* NW_ABI_VERSION the library was built with. */
int nw_abi_version(void);

#ifdef __cplusplus
}
#endif

#endif /* NWCRYPTO_H */
