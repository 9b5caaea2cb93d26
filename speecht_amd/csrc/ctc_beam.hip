// CTC prefix beam search (top path) on gfx950 -- SURVEY 8(f) item 3, BASELINE config 5 -- without a scorer, and with the word
// n-gram scorer of the reference's decoder (ctc_beam_kernel<.., LM = true>, st_ctc_beam_search_decode_lm), also for several
// weight triples in one launch (a grid of utterances x candidates, st_ctc_beam_search_decode_lm_candidates: the LM weight search).
// Both searches also run carried across the steps of a live stream (ctc_beam_kernel<.., STREAM = true>, ctc_beam_read_kernel;
// st_ctc_beam_stream_step / _read): the same frame loop between a load and a save of the beam's state.
// Hotword biasing (ctc_beam_kernel<.., BIAS = true>, st_ctc_beam_search_decode_bias_nbest / _lm_bias_nbest) is a second scorer of the
// LM's shape: a table-driven automaton over the labels whose state is a function of the prefix alone (BiasArgs below).
// The biased searches run carried across steps too (ctc_beam_kernel<.., STREAM, BIAS>, ctc_beam_read_kernel<.., BIAS>;
// st_ctc_beam_stream_step_bias / _read_bias / _step_pieces_bias), each stream starting in a root state of its own (roots[]).
//
// The reference reaches a beam search only through its KenLM TensorFlow fork (speech_model.py:101-111);
// this kernel follows the stock tf.nn.ctc_beam_search_decoder recursion, with the candidate order of
// oracle/w2l_oracle.py::ctc_beam_search_decode (total desc, slot*C + c asc); the scorer's hooks follow tests/lm_oracle.py.
//
// Mapping: ONE wavefront per utterance (the recursion is sequential in time, utterances are the
// parallel axis), so a frame is a chain of dependent steps on one wave and its length IS the decode time
// (round 2: 13 300 cycles per frame, measured per phase with s_memtime; round 3: the chain below).
// What does not depend on the beam is taken off the chain: the log-softmax of every frame is computed by a
// fully parallel kernel first (same wave reductions, bit-identical values) and read one frame ahead.
// Everything that lives across frames -- the beam entries -- sits in LDS, double buffered; a frame is:
// parent matching (W^2 hash compares spread over the lanes, all LDS reads of the four passes issued before the
// first compare), the stay candidates, one sortable 32-bit score per candidate (W*C of them, lane-strided, in
// registers; branch-free, three LDS reads each), and a wave-parallel selection of the W best: the W-th largest
// LANE maximum -- found by a 32-step radix select on ballots, not by ranking the lanes -- bounds the W-th largest
// candidate from below, the few candidates at or above it are compacted into LDS and ranked by counting
// (sequential maximum rounds remain for the rare case of more than 64 survivors).  Prefix identity is a
// 64-bit mixed hash + length (the trie TF keeps in host memory would be a pointer chase per candidate);
// the emitted labels are recorded as (parent node, label) pairs in a per-utterance pool whose slot is a
// pure function of (frame, rank), so there are no atomics and the result is deterministic.
#include <math.h>

#include "ctc_lattice.h"
#include "lm_tables.h"
#include "st_common.h"

namespace {

using st::RowMap;
constexpr int kMaxBeam = 128;          // beams of 65..128 (the reference's operating point is 100) run the WIDE instantiation
constexpr int kMaxClasses = 32;
constexpr unsigned long long kRootHash = 0x243F6A8885A308D3ull;

template <int MAXB>
struct BeamSet {   // structure of arrays: lane r reads/writes entry r without bank conflicts
  unsigned long long hash[MAXB];
  unsigned long long parent_hash[MAXB];
  int len[MAXB];
  int last[MAXB];
  int node[MAXB];
  float pb[MAXB];
  float pl[MAXB];
  float total[MAXB];
};

// ---- word n-gram scorer of the LM-scored search (TF ctc_beam_search.h scorer hooks; the semantics: tests/lm_oracle.py) --------
// An entry's LM state is a pure function of its prefix, and so are its 28 expansion deltas (score of the child - score of the
// entry, labels a-z ' and space): they are computed ONCE, when the entry enters the beam -- one trie-row read and one n-gram
// query -- and kept in LDS beside it; the scoring pass reads delta[slot][c] the way it reads lp_s[c].  "score" = lm_score (the
// words so far) + the lowest unigram of the incomplete word's completions (`wpart`; oov_score once the prefix has left the
// vocabulary, 0 at a word start), so the deltas are differences of small numbers, never of the running sums.
constexpr int kSpace = 27;                 // vocabulary.SPACE_ID; the classes of an LM search are a-z ' space blank (C = 29)
constexpr int kCtx = stlm::kMaxOrder - 1;  // context words kept per entry
constexpr int kDeltaPitch = 32;

struct LmParams {
  const stlm::View& v;  // device tables (the kernel argument's: a copy indexed by order would live in scratch)
  float lm_weight, word_count_weight, valid_word_count_weight, oov_score;
};

// The scorer's kernel argument: the tables and up to kLaunchCandidates weight triples {lm, word count, valid word count}; the
// block (utterance b, candidate blockIdx.y) decodes with triple blockIdx.y.  The triples travel in the kernel arguments (with the
// tables 1 208 of the 4 096 argument bytes), so a launch takes at most kLaunchCandidates of them and the host splits larger
// requests.
constexpr int kLaunchCandidates = 64;
struct LmArgs {
  stlm::View v;
  float oov_score;
  float w[kLaunchCandidates][3];
};

template <int MAXB>
struct LmSet {        // structure of arrays, like BeamSet
  int ctx[kCtx][MAXB];      // the last n_ctx word ids, oldest first
  int n_ctx[MAXB];
  int node[MAXB];           // trie node of the incomplete word, -1 once it has left the vocabulary
  unsigned mask[MAXB];      // that node's child mask / first child / terminal word id (0 / 0 / -1 for -1)
  int first[MAXB];
  int word[MAXB];
  float wpart[MAXB];        // score - lm_score
  float dself[MAXB];        // score - the parent's score (the stay candidate's parent inflow)
};

// the node record of `node` (a global read; -1: no node)
__device__ __forceinline__ stlm::TrieNode lm_node(const LmParams& P, int node) {
  if (node < 0) return stlm::TrieNode{0u, 0, P.oov_score, -1};
  return P.v.trie[node];
}

// the expansion deltas of an entry in state (node record nd, context, wpart) into an LDS row of kDeltaPitch floats: the children's
// lowest unigrams (one read each, all independent) and, for space, the incomplete word against the context
__device__ __forceinline__ void lm_deltas(const LmParams& P, const stlm::TrieNode& nd, const int* ctx, int n_ctx, float wpart,
                                          float* row) {
  float m[stlm::kLetters];
#pragma unroll
  for (int c = 0; c < stlm::kLetters; ++c) {
    const bool has = (nd.mask >> c) & 1u;
    const int child = nd.first + __builtin_popcount(nd.mask & ((1u << c) - 1u));
    m[c] = has ? P.v.trie[child].min_logp : P.oov_score;
  }
  const int w = nd.word >= 0 ? nd.word : stlm::kUnk;
  const float ws = stlm::score(P.v, ctx, n_ctx, w) + P.word_count_weight + (nd.word >= 0 ? P.valid_word_count_weight : 0.f);
  float4* r4 = reinterpret_cast<float4*>(row);
#pragma unroll
  for (int q = 0; q < 6; ++q) r4[q] = make_float4(m[4 * q] - wpart, m[4 * q + 1] - wpart, m[4 * q + 2] - wpart, m[4 * q + 3] - wpart);
  r4[6] = make_float4(m[24] - wpart, m[25] - wpart, m[26] - wpart, ws - wpart);
  r4[7] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// appends word w to a context of n_ctx words holding at most cap (oldest dropped); compile-time indices only (no scratch)
__device__ __forceinline__ void push_ctx(int (&ctx)[kCtx], int& n_ctx, int cap, int w) {
  if (cap <= 0) return;
  const bool full = n_ctx == cap;
#pragma unroll
  for (int i = 0; i < kCtx; ++i) {
    const int shifted = i + 1 < kCtx ? ctx[i + 1] : w;
    ctx[i] = full ? (i == cap - 1 ? w : (i < cap - 1 ? shifted : ctx[i])) : (i == n_ctx ? w : ctx[i]);
  }
  n_ctx = full ? n_ctx : n_ctx + 1;
}

// entry e of the new set, made from parent entry `slot` of the old set by label c (stay: c is blank): its LM state, and -- for
// a child -- its expansion deltas (the trie node record, then the children's row and the n-gram query of the word it spells)
template <int MAXB>
__device__ __forceinline__ void lm_enter(const LmParams& P, const LmSet<MAXB>& SL, LmSet<MAXB>& NL, const float* prow, float* row,
                                         int slot, int e, int c, bool stay) {
  int ctx[kCtx];
#pragma unroll
  for (int i = 0; i < kCtx; ++i) ctx[i] = SL.ctx[i][slot];
  int nc = SL.n_ctx[slot];
  if (stay) {
#pragma unroll
    for (int q = 0; q < kDeltaPitch / 4; ++q) reinterpret_cast<float4*>(row)[q] = reinterpret_cast<const float4*>(prow)[q];
    NL.node[e] = SL.node[slot]; NL.mask[e] = SL.mask[slot]; NL.first[e] = SL.first[slot]; NL.word[e] = SL.word[slot];
    NL.wpart[e] = SL.wpart[slot]; NL.dself[e] = SL.dself[slot];
  } else {
    int node;
    if (c == kSpace) {
      // the incomplete word (or <unk>) shifts into the context; the trie resets to the root
      push_ctx(ctx, nc, P.v.order - 1, SL.word[slot] >= 0 ? SL.word[slot] : stlm::kUnk);
      node = 0;
    } else {
      const unsigned pm = SL.mask[slot];
      node = (SL.node[slot] >= 0 && ((pm >> c) & 1u)) ? SL.first[slot] + __builtin_popcount(pm & ((1u << c) - 1u)) : -1;
    }
    const stlm::TrieNode nd = lm_node(P, node);
    const float wpart = c == kSpace ? 0.f : nd.min_logp;
    NL.node[e] = node; NL.mask[e] = nd.mask; NL.first[e] = nd.first; NL.word[e] = nd.word;
    NL.wpart[e] = wpart; NL.dself[e] = prow[c];
    lm_deltas(P, nd, ctx, nc, wpart, row);
  }
#pragma unroll
  for (int i = 0; i < kCtx; ++i) NL.ctx[i][e] = ctx[i];
  NL.n_ctx[e] = nc;
}

// end of utterance: entry e scores its incomplete word (if non-empty) and then </s>; returns its total after that.  ONE function
// for the whole-utterance tail and the stream's read-out (L and row in LDS there, in the state record here), so that both compile
// the same operations: the two results are compared bit for bit.
template <int MAXB>
__device__ __forceinline__ float lm_final_total(const LmParams& P, const LmSet<MAXB>& L, const float* row, float total, int e) {
  int ctx[kCtx];
#pragma unroll
  for (int i = 0; i < kCtx; ++i) ctx[i] = L.ctx[i][e];
  int nc = L.n_ctx[e];
  float d = -L.wpart[e];
  if (L.node[e] != 0) {
    d = row[kSpace];
    push_ctx(ctx, nc, P.v.order - 1, L.word[e] >= 0 ? L.word[e] : stlm::kUnk);
  }
  d += stlm::score(P.v, ctx, nc, stlm::kEos);
  return total + P.lm_weight * d;
}

__device__ __forceinline__ unsigned long long child_hash(unsigned long long h, int c) {
  unsigned long long x = h + 0x9E3779B97F4A7C15ull * (unsigned long long)(c + 1);
  x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27; x *= 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ float lse(float a, float b) {
  // hardware exp2 / log2 (1 ulp): the two calls sit on the per-frame dependent chain of the search, and the libm forms
  // (range reduction + polynomial, ~40 instructions each) were a fifth of the `stay` phase; the result differs from them
  // by < 2e-7, far inside the 1e-4 the scores are held to
  float hi = fmaxf(a, b), lo = fminf(a, b);
  return hi == -INFINITY ? -INFINITY : hi + __logf(1.f + __expf(lo - hi));
}

// ---- wave64 reductions on the DPP network (row shifts + row broadcasts; no LDS round trips) --------
template <int CTRL, int ROW_MASK, bool ZERO_INVALID>
__device__ __forceinline__ int dpp_i32(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, CTRL, ROW_MASK, 0xf, ZERO_INVALID);
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#define ST_STEP(CTRL) v = max(v, (unsigned)dpp_i32<CTRL, 0xf, false>((int)v, (int)v))   /* invalid source lane -> own value */
  ST_STEP(0x111); ST_STEP(0x112); ST_STEP(0x114); ST_STEP(0x118);   // row_shr 1, 2, 4, 8: lane 15 of a row = row maximum
  ST_STEP(0x142); ST_STEP(0x143);                                   // row_bcast 15, 31: lane 63 = wave maximum
#undef ST_STEP
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ unsigned wave_min_u32(unsigned v) {
#define ST_STEP(CTRL) v = min(v, (unsigned)dpp_i32<CTRL, 0xf, false>((int)v, (int)v))
  ST_STEP(0x111); ST_STEP(0x112); ST_STEP(0x114); ST_STEP(0x118); ST_STEP(0x142); ST_STEP(0x143);
#undef ST_STEP
  return (unsigned)__builtin_amdgcn_readlane((int)v, 63);
}
__device__ __forceinline__ float wave_max_f32(float v) {
#define ST_STEP(CTRL) v = fmaxf(v, __int_as_float(dpp_i32<CTRL, 0xf, false>(__float_as_int(v), __float_as_int(v))))
  ST_STEP(0x111); ST_STEP(0x112); ST_STEP(0x114); ST_STEP(0x118); ST_STEP(0x142); ST_STEP(0x143);
#undef ST_STEP
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_sum_f32(float v) {
#define ST_STEP(CTRL, MASK) v += __int_as_float(dpp_i32<CTRL, MASK, true>(0, __float_as_int(v)))
  ST_STEP(0x111, 0xf); ST_STEP(0x112, 0xf); ST_STEP(0x114, 0xf); ST_STEP(0x118, 0xf);   // scan inside each row
  ST_STEP(0x142, 0xa); ST_STEP(0x143, 0xc);                                            // fold rows into lane 63
#undef ST_STEP
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// inclusive prefix sum over the wave (lane 63 holds the total)
__device__ __forceinline__ int wave_incl_scan_i32(int v) {
#define ST_STEP(CTRL, MASK) v += dpp_i32<CTRL, MASK, true>(0, v)
  ST_STEP(0x111, 0xf); ST_STEP(0x112, 0xf); ST_STEP(0x114, 0xf); ST_STEP(0x118, 0xf);   // scan inside each row of 16
  ST_STEP(0x142, 0xa); ST_STEP(0x143, 0xc);                                            // carry the rows' totals up
#undef ST_STEP
  return v;
}

// monotone map float -> unsigned (larger float, larger integer) and back
__device__ __forceinline__ unsigned order_bits(float v) {
  const unsigned bits = (unsigned)__float_as_int(v);
  return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
constexpr unsigned kOrdNegInf = 0x007FFFFFu;      // order_bits(-inf)
__device__ __forceinline__ float order_value(unsigned ord) {
  return __int_as_float((int)(ord ^ ((ord >> 31) ? 0x80000000u : 0xFFFFFFFFu)));
}

// log-softmax of every frame, one wavefront per frame: out[(b * T + t) * 32 + c] (0 for c >= C).  The same wave reductions
// in the same order as the search kernel used when it did this inside its frame loop, so the values are bit-identical;
// frames at or beyond an utterance's length are skipped.
// transform 1: the decoder's input is tf.log(tf.nn.softmax(logits) + 1e-8) / log(10) -- what the reference hands its beam search
// (speech_model.py:102) -- and the decoder then normalises THAT per frame like any other input (ctc_beam_search.h Step).
// one row by one wave: x is lane's logit (-inf for lane >= C), the row goes to out[0 .. 32)
__device__ __forceinline__ void logsoftmax_row(float x, int lane, int C, int transform, float* __restrict__ out) {
  const float m = wave_max_f32(x);
  const float z = wave_sum_f32(lane < C ? expf(x - m) : 0.f);
  if (transform == 1) {
    // in double (off the search's chain, one wave per frame): the transform flattens the distribution (a temperature of ln 10),
    // near-ties at the beam boundary get closer, and the stored row should be the fp32 rounding of the exact value
    auto wsum = [](double v) {
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
      return v;
    };
    const double e = lane < C ? exp((double)x - (double)m) : 0.0;
    const double zz = wsum(e);
    const double xt = lane < C ? log10(e / zz + 1e-8) : -INFINITY;
    const float mt = wave_max_f32((float)xt);                       // any value near the maximum centres the sum
    const double z2 = wsum(lane < C ? exp(xt - (double)mt) : 0.0);
    if (lane < kMaxClasses) out[lane] = lane < C ? (float)(xt - (double)mt - log(z2)) : 0.f;
    return;
  }
  if (lane < kMaxClasses) out[lane] = lane < C ? x - m - logf(z) : 0.f;
}

__global__ __launch_bounds__(256) void logsoftmax_rows_kernel(const float* __restrict__ logits, RowMap map, int T, int C,
                                                              const int* __restrict__ seq_lens, int transform, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, b = blockIdx.y;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= min(seq_lens[b], T)) return;
  const float x = lane < C ? logits[map.off(b, t) + lane] : -INFINITY;
  logsoftmax_row(x, lane, C, transform, out + ((long)b * T + t) * kMaxClasses);
}

// ... and of the rows of one streaming step, row r of the launch at logits[r * pitch]: out[r * 32 + c]
__global__ __launch_bounds__(256) void logsoftmax_step_rows_kernel(const float* __restrict__ logits, int pitch, int n_rows, int C,
                                                                   int transform, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= n_rows) return;
  const float x = lane < C ? logits[(long)r * pitch + lane] : -INFINITY;
  logsoftmax_row(x, lane, C, transform, out + (long)r * kMaxClasses);
}

// The search kernel runs ONE wavefront per workgroup, and a wave's LDS operations execute in order: between its phases it
// needs no s_barrier, only the compiler kept from moving LDS accesses across the phase boundary and the LDS queue drained.
// __syncthreads() would also wait for vmcnt(0) -- i.e. for the next frame's log-probabilities, whose load is meant to stay
// in flight under this frame's work.
#define ST_WAVE_SYNC() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

// CPL = candidates per lane (beam_width * C <= 64 * CPL).  MAXB = 64: candidate k = lane + 64 j is (slot, class) = (k / C, k % C).
// MAXB = 128 (WIDE, beams of 65..128; CPL = 64): the classes take a pitch of 32 -- k = slot * 32 + class, the same order between live
// candidates -- so a lane's class is lane & 31 for all its candidates and its slots are (lane >> 5) + 2 j: no division, no index
// arrays; two beam entries per lane in the per-entry phases; the selection bound is the exact W-th largest score (a bitwise binary
// search over the sortable scores: 32 wave-parallel counts) instead of the lane / pair / quad maxima, which bound only 64.
// LM: the word n-gram scorer (LmParams) enters through the expansion deltas; LM = false compiles to the LM-free search.
// NBEST: the tail writes the n_best best final entries (NbestArgs) instead of the top path; the frame loop is the same code, and
// NBEST = false compiles to the top-path kernel (its NbestArgs is empty).
template <bool NBEST>
struct NbestArgs {};
template <>
struct NbestArgs<true> {
  int n_best;          // 1 <= n_best <= W; the outputs are [utterance][n_best](...)
  int* n_hyps;         // [utterance]: min(n_best, entries alive)
};

// STREAM: the search carried across steps (st_ctc_beam_stream_step).  Block b is stream b; it starts from the stream's state
// record instead of the root (from the root when the table row says reset), decodes the stream's rows of this step -- lp_all holds
// the log-softmax rows of the STEP, row r of the launch at lp_all[r * 32] -- numbers its nodes with the absolute frame index, so
// that the chains are those of the whole-utterance search, saves the state again and has no tail (ctc_beam_read_kernel reads the
// hypothesis out).  A frame whose nodes would lie beyond the stream's pool is not decoded: the record's status word says so.
// STREAM = false compiles to the kernels above (its StreamArgs is empty).
struct StreamHeader {     // the first kStateHeader bytes of a state record
  int magic;              // stream_magic(W, LM) once the record has been reset by a launch of this beam width and kind
  int nb;                 // live entries
  int frames;             // frames decoded so far
  int status;             // kPoolFull: a frame was refused
  int stable_len;         // labels every live entry shares (kept by the read-out)
  int pad;
  double offset;
};
constexpr int kStateHeader = 32;
constexpr int kPoolFull = 1;
static_assert(sizeof(StreamHeader) == kStateHeader, "state record header");
// (bit 12: a hotword-biased search -- its records carry two more arrays, and neither kind continues the other's)
__host__ __device__ constexpr int stream_magic(int W, bool lm, bool bias = false) {
  return 0x53420000 | (bias ? 0x1000 : 0) | (W << 1) | (lm ? 1 : 0);
}
// record: [header | BeamSet<MAXB> | LM: LmSet<MAXB>, deltas [MAXB][kDeltaPitch] | BIAS: hotword states int [MAXB], bself float [MAXB]]
template <int MAXB>
constexpr size_t stream_state_bytes(bool lm) {
  return kStateHeader + sizeof(BeamSet<MAXB>) + (lm ? sizeof(LmSet<MAXB>) + sizeof(float) * MAXB * kDeltaPitch : 0);
}
template <int MAXB>
constexpr size_t stream_bias_state_bytes(bool lm) {
  return stream_state_bytes<MAXB>(lm) + (sizeof(int) + sizeof(float)) * MAXB;
}

template <bool STREAM>
struct StreamArgs {};
template <>
struct StreamArgs<true> {
  const int* rows;        // [n_rows][2] (stream, absolute frame) of the step
  const int* table;       // [streams][4] {first row, rows, decode limit or -1, reset}
  char* state;            // [streams] records of state_stride bytes
  long state_stride;
  int max_frames;         // the pool holds max_frames * W + 1 nodes per stream
};

// BIAS: hotword biasing.  The phrases' trie is an automaton over the labels (semantics: include/speecht_hip.h,
// tests/hotword_oracle.py), tabulated by the host: next[n][32] / gain[n][32] / fin[n] in global memory.  An entry carries its state and
// `bself`, the gain it was entered with (double buffered beside the sets); the scorer enters the frame loop where the LM does: a child
// candidate adds gain[state(slot)][c], the stay candidate's parent inflow adds bself[e], the tail adds fin[state(e)] before ranking.
// The gain rows are read from the GLOBAL table in the scoring pass (one LDS read of the slot's state, then one load per candidate,
// all issued with the pass's LDS reads; the table of a phrase list is a few hundred KB and stays in L2): copies of the rows in LDS,
// as the LM deltas have, would cost 32 KB more at MAXB = 128 and a 128-byte copy per entry and frame for a row that, unlike the LM's,
// costs nothing to look up again.  Every state written to LDS is clamped to [0, n_states): a malformed table gives wrong text, never
// a read outside the tables.  BIAS = false compiles to the kernels above (its BiasArgs is empty).
// STREAM && BIAS: the entries' states and bself are saved in the record behind the other parts and restored from it; a search that
// starts afresh (the stream's first step, a reset of an endpointed piece) starts in state roots[stream], not 0 -- the tables may hold
// several phrase sets one after the other, each set's `next` pointing into its own rows, and roots[s] is the first row of stream s's.
template <bool BIAS, bool STREAM = false>
struct BiasArgs {};
template <>
struct BiasArgs<true, false> {
  const int* next;        // [n_states][kBiasPitch]
  const float* gain;      // [n_states][kBiasPitch]
  const float* fin;       // [n_states]
  int n_states;
};
template <>
struct BiasArgs<true, true> : BiasArgs<true, false> {
  const int* roots;       // [streams]
};
constexpr int kBiasPitch = 32;

// words of 4 bytes between LDS and a state record, lane-strided
__device__ __forceinline__ void copy_words(void* dst, const void* src, int bytes, int lane) {
  int* d = static_cast<int*>(dst);
  const int* s = static_cast<const int*>(src);
  for (int i = lane; i < bytes / 4; i += 64) d[i] = s[i];
}

template <int CPL, int MAXB, bool LM, bool NBEST = false, bool STREAM = false, bool BIAS = false>
__global__ __launch_bounds__(64) void ctc_beam_kernel(const float* __restrict__ lp_all, int T, int C,
                                                      const int* __restrict__ seq_lens, int W,
                                                      int2* __restrict__ node_pool, long pool_stride,
                                                      int* __restrict__ ids, int max_out,
                                                      int* __restrict__ out_lens, float* __restrict__ out_logp, LmArgs lma,
                                                      NbestArgs<NBEST> nx, StreamArgs<STREAM> sx = {},
                                                      BiasArgs<BIAS, BIAS && STREAM> bx = {}) {
  static_assert(!(NBEST && STREAM), "a stream has no N-best lists");
  static_assert(!BIAS || NBEST || STREAM, "hotwords: the N-best and the stream instantiations only (the top path is the n_best = 1 list)");
  constexpr bool WIDE = MAXB > 64;
  constexpr int SURV = WIDE ? 256 : 128;             // capacity of the fast selection; more survivors take the sequential rounds
  static_assert(MAXB == 64 || (MAXB == 128 && CPL == 64), "wide beams: 128 entries x 32 class slots = 64 candidates per lane");
  __shared__ BeamSet<MAXB> sets[2];
  __shared__ float lp_s[kMaxClasses];
  // per beam entry, for the scoring pass: {total, p_blank of the previous frame, total of the stay candidate, last label}
  __shared__ __attribute__((aligned(16))) float4 slot_s[MAXB];
  __shared__ float stay_pb[MAXB], stay_pl[MAXB];
  __shared__ int parent_of[MAXB];
  __shared__ unsigned dead[MAXB];
  __shared__ int sel_k[MAXB];
  __shared__ __attribute__((aligned(16))) unsigned long long surv[SURV + 16];   // compacted survivor keys of the fast selection (+ zero pad)
  __shared__ float sel_v[MAXB];
  // LM state and expansion deltas of the entries (double buffered with the sets; a single element when LM is off)
  constexpr int LMB = LM ? MAXB : 1;
  __shared__ LmSet<LMB> lms[2];
  __shared__ __attribute__((aligned(16))) float delta_s[2][LMB][kDeltaPitch];
  // hotword state and entry gain of the entries (double buffered with the sets; a single element when BIAS is off)
  constexpr int BB = BIAS ? MAXB : 1;
  __shared__ int bstate_s[2][BB];
  __shared__ float bself_s[2][BB];

  const int b = blockIdx.x, lane = threadIdx.x;
  // LM: the candidate axis -- blockIdx.y picks the weight triple, its own node pool and its own output rows
  const int p = LM ? (int)blockIdx.y : 0;
  const LmParams lmp{lma.v, lma.w[p][0], lma.w[p][1], lma.w[p][2], lma.oov_score};
  const long ob = LM ? (long)p * gridDim.x + b : b;
  const float lw = lmp.lm_weight;
  // STREAM: the frames of this step (Tb of them, the first at row `first` of the launch) continue the t0 frames decoded before
  int Tb, t0 = 0, first = 0, status = 0;
  bool fresh = true;
  [[maybe_unused]] StreamHeader* hdr = nullptr;
  if constexpr (STREAM) {
    hdr = reinterpret_cast<StreamHeader*>(sx.state + b * sx.state_stride);
    first = sx.table[4 * b];
    const int count = sx.table[4 * b + 1], limit = sx.table[4 * b + 2];
    fresh = sx.table[4 * b + 3] != 0;
    if (!fresh && hdr->magic != stream_magic(W, LM, BIAS)) return;     // never reset for this search: nothing to continue
    if (!fresh) { t0 = hdr->frames; status = hdr->status; }
    Tb = count;
    if (limit >= 0 && count > 0) Tb = max(min(count, limit - sx.rows[2 * first + 1]), 0);   // rows at or past the limit
    if (Tb > sx.max_frames - t0) {                                                        // ... or past the pool
      Tb = max(sx.max_frames - t0, 0);
      status |= kPoolFull;
    }
    if (!fresh && Tb == 0) {                                     // nothing to decode: the record stays as it is
      if (lane == 0 && status != hdr->status) hdr->status = status;
      return;
    }
  } else {
    Tb = min(seq_lens[b], T);
  }
  const int blank = C - 1;
  int2* nodes = node_pool + ob * pool_stride;

  // (slot, class) of this lane's candidates k = lane + 64 j: fixed for the whole utterance
  constexpr int NIDX = WIDE ? 1 : CPL;               // (wide beams compute them on the fly: slot (lane >> 5) + 2 j, class lane & 31)
  int cslot[NIDX], ccls[NIDX];
#pragma unroll
  for (int j = 0; j < NIDX; ++j) {
    int k = lane + 64 * j;
    cslot[j] = k / C;
    ccls[j] = k - cslot[j] * C;
  }
  const int wslot0 = lane >> 5, wcls = lane & 31;

  int cur = 0, nb = 1;
  double offset = 0.0;                   // log-probability of the current best entry (wave-uniform)
  if constexpr (STREAM) {
    if (!fresh) {
      const char* rec = sx.state + b * sx.state_stride;
      nb = min(max(hdr->nb, 0), W);
      offset = hdr->offset;
      copy_words(&sets[0], rec + kStateHeader, sizeof(BeamSet<MAXB>), lane);
      if constexpr (LM) {
        copy_words(&lms[0], rec + kStateHeader + sizeof(BeamSet<MAXB>), sizeof(LmSet<MAXB>), lane);
        copy_words(&delta_s[0][0][0], rec + kStateHeader + sizeof(BeamSet<MAXB>) + sizeof(LmSet<MAXB>),
                   sizeof(float) * MAXB * kDeltaPitch, lane);
      }
      if constexpr (BIAS) {
        // (clamped like every state written to LDS: whatever the record holds, no read leaves the tables)
        const int* saved = reinterpret_cast<const int*>(rec + stream_state_bytes<MAXB>(LM));
        for (int e = lane; e < MAXB; e += 64) bstate_s[0][e] = min(max(saved[e], 0), bx.n_states - 1);
        copy_words(&bself_s[0][0], rec + stream_state_bytes<MAXB>(LM) + sizeof(int) * MAXB, sizeof(float) * MAXB, lane);
      }
    }
  }
  if (lane == 0 && fresh) {
    BeamSet<MAXB>& s = sets[0];
    s.hash[0] = kRootHash; s.parent_hash[0] = 0; s.len[0] = 0; s.last[0] = -1; s.node[0] = 0;
    s.pb[0] = 0.f; s.pl[0] = -INFINITY; s.total[0] = 0.f;
    if constexpr (BIAS) {
      int root = 0;
      if constexpr (STREAM) root = min(max(bx.roots[b], 0), bx.n_states - 1);
      bstate_s[0][0] = root;
      bself_s[0][0] = 0.f;
    }
    if constexpr (LM) {
      // root: context <s>, the trie root, lm_score = score = 0
      LmSet<LMB>& L = lms[0];
      const int nc = min(1, lmp.v.order - 1);
      L.ctx[0][0] = stlm::kBos;
      L.n_ctx[0] = nc;
      const stlm::TrieNode nd = lm_node(lmp, 0);
      L.node[0] = 0; L.mask[0] = nd.mask; L.first[0] = nd.first; L.word[0] = nd.word;
      L.wpart[0] = 0.f; L.dself[0] = 0.f;
      const int bos = stlm::kBos;
      lm_deltas(lmp, nd, &bos, nc, 0.f, delta_s[0][0]);
    }
  }
  __syncthreads();

  // log-softmax rows of this utterance, written by logsoftmax_rows_kernel: [t][32]
  const float* __restrict__ lp_rows = lp_all + (STREAM ? (long)first : (long)b * T) * kMaxClasses;
  float lp_next = (lane < kMaxClasses && Tb > 0) ? lp_rows[lane] : 0.f;
  for (int t = 0; t < Tb; ++t) {
    const BeamSet<MAXB>& S = sets[cur];
    BeamSet<MAXB>& N = sets[cur ^ 1];
    // (1) this frame's log-probabilities into LDS; the next frame's row is already on its way
    if (lane < kMaxClasses) lp_s[lane] = lp_next;
    if (t + 1 < Tb && lane < kMaxClasses) lp_next = lp_rows[(long)(t + 1) * kMaxClasses + lane];
#pragma unroll
    for (int e = lane; e < MAXB; e += 64) {
      parent_of[e] = -1;
      dead[e] = 0u;
    }
    ST_WAVE_SYNC();
    // (2) which entries have their parent prefix in the beam?  (e, p) pairs spread over the lanes; the LDS reads of all
    // passes are issued before the first compare (a pass at a time each one waits a full LDS round trip)
    if constexpr (WIDE) {
      // two entries per lane against every candidate parent p in turn (broadcast reads of p's fields); prefix identity is
      // unique in the beam, so an entry matches at most one p
      int len_e[2], last_e[2];
      unsigned long long he[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int e = lane + 64 * i;
        const bool in = e < nb;
        len_e[i] = in ? S.len[e] : -7;
        he[i] = S.parent_hash[in ? e : 0];
        last_e[i] = S.last[in ? e : 0];
      }
#pragma unroll 4
      for (int p = 0; p < nb; ++p) {
        const int len_p = S.len[p];
        const unsigned long long hp = S.hash[p];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if (len_p + 1 == len_e[i] && hp == he[i]) {
            parent_of[lane + 64 * i] = p;
            atomicOr(&dead[p], 1u << last_e[i]);
          }
        }
      }
    } else {
      int lg = 32 - __clz(max(nb - 1, 1));
      if (nb <= 1) lg = 0;
      const int wp = 1 << lg, pairs = nb << lg;
      constexpr int PASSES = 4;                      // 64 * 4 = 16 x 16 pairs; wider beams loop
      if (wp <= 64 && pairs <= 64 * PASSES) {
        // p = lane & (wp - 1) for every pass: the candidate parent's fields are read once
        const int p = lane & (wp - 1);
        const bool p_in = p < nb;
        const int len_p = S.len[p_in ? p : 0];
        const unsigned long long hp = S.hash[p_in ? p : 0];
        int e_[PASSES], len_e[PASSES], last_e[PASSES];
        unsigned long long he[PASSES];
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
          const int idx = lane + 64 * i;
          const bool in = idx < pairs && p_in;
          e_[i] = in ? idx >> lg : 0;
          len_e[i] = in ? S.len[e_[i]] : -7;
          he[i] = S.parent_hash[e_[i]];
          last_e[i] = S.last[e_[i]];
        }
#pragma unroll
        for (int i = 0; i < PASSES; ++i) {
          if (len_p + 1 == len_e[i] && hp == he[i]) {
            parent_of[e_[i]] = p;
            atomicOr(&dead[p], 1u << last_e[i]);         // child (p, last[e]) already exists: merged into e's stay
          }
        }
      } else {
        for (int idx = lane; idx < pairs; idx += 64) {
          const int e = idx >> lg, p = idx & (wp - 1);
          if (p < nb && S.len[p] + 1 == S.len[e] && S.hash[p] == S.parent_hash[e]) {
            parent_of[e] = p;
            atomicOr(&dead[p], 1u << S.last[e]);
          }
        }
      }
    }
    ST_WAVE_SYNC();
    // (2b) the stay candidate of entry `lane` (wide beams: and of entry lane + 64)
#pragma unroll
    for (int e = lane; e < MAXB; e += 64) {
      if (e >= nb) break;
      // every LDS read up front (own fields, then the parent's through a clamped index), the arithmetic behind them
      const float tot = S.total[e], pl0 = S.pl[e], pb0 = S.pb[e];
      const int len0 = S.len[e], last0 = S.last[e], p = parent_of[e];
      const float lp_blank = lp_s[blank], lp_last = lp_s[max(last0, 0)];
      const int pc = max(p, 0);
      const int plen = S.len[pc], plast = S.last[pc];
      const float ppb = S.pb[pc], ptot = S.total[pc];
      const float npb = tot + lp_blank;
      float npl = -INFINITY;
      if (len0 > 0) {
        float mass = pl0;
        if constexpr (BIAS) {
          float inflow = (plen > 0 && plast == last0) ? ppb : ptot;
          if constexpr (LM) inflow += lw * lms[cur].dself[e];
          if (p >= 0) mass = lse(mass, inflow + bself_s[cur][e]);
        } else if constexpr (LM) {
          if (p >= 0) mass = lse(mass, ((plen > 0 && plast == last0) ? ppb : ptot) + lw * lms[cur].dself[e]);
        } else {
          if (p >= 0) mass = lse(mass, (plen > 0 && plast == last0) ? ppb : ptot);
        }
        npl = mass + lp_last;
      }
      stay_pb[e] = npb;
      stay_pl[e] = npl;
      slot_s[e] = make_float4(tot, pb0, lse(npb, npl), __int_as_float(last0));
    }
    ST_WAVE_SYNC();
    // (3) one sortable 32-bit score per candidate, in registers (candidate index k = lane + 64 j is implicit)
    unsigned ord[CPL];
    unsigned best_ord = 0u;                               // 0 is below every real candidate
    int best_j = 0;
    if constexpr (!WIDE) {
      // all reads first (three per candidate, none behind a branch), then the arithmetic
      float4 info[CPL];
      unsigned dd[CPL];
      float lpc[CPL];
      float dl[LM ? CPL : 1];
      [[maybe_unused]] float bg[BIAS ? CPL : 1];
      if constexpr (BIAS) {
        // the gains first: a global load behind an LDS read, in flight under the LDS reads below
#pragma unroll
        for (int j = 0; j < CPL; ++j) bg[j] = bx.gain[bstate_s[cur][cslot[j] < nb ? cslot[j] : 0] * kBiasPitch + ccls[j]];
      }
#pragma unroll
      for (int j = 0; j < CPL; ++j) {
        const int sl = cslot[j] < nb ? cslot[j] : 0;
        info[j] = slot_s[sl];
        dd[j] = dead[sl];
        lpc[j] = lp_s[ccls[j]];
        if constexpr (LM) dl[j] = delta_s[cur][sl][ccls[j]];
      }
#pragma unroll
      for (int j = CPL - 1; j >= 0; --j) {                // descending j + ">=": the lowest j wins a tie
        const int c = ccls[j];
        float child;
        if constexpr (BIAS) {
          float base = (__float_as_int(info[j].w) == c) ? info[j].y : info[j].x;
          if constexpr (LM) base += lw * dl[j];
          child = ((dd[j] >> c) & 1u) ? -INFINITY : (base + bg[j]) + lpc[j];
        } else if constexpr (LM)                             // TF GetStateExpansionScore(child state, previous)
          child = ((dd[j] >> c) & 1u) ? -INFINITY : (((__float_as_int(info[j].w) == c) ? info[j].y : info[j].x) + lw * dl[j]) + lpc[j];
        else
          child = ((dd[j] >> c) & 1u) ? -INFINITY : ((__float_as_int(info[j].w) == c) ? info[j].y : info[j].x) + lpc[j];
        const float v = c == blank ? info[j].z : child;
        const unsigned oj = cslot[j] < nb ? order_bits(v) : 0u;
        ord[j] = oj;
        if (oj >= best_ord) { best_ord = oj; best_j = j; }
      }
    } else {
      // one class per lane (the 32 lanes of a half read the same entry: broadcast reads), eight entries at a time
      const int c = wcls;
      const float lpc = lp_s[c];
      const bool cls_live = c < C;
#pragma unroll
      for (int j0 = 0; j0 < CPL; j0 += 8) {
        float4 info[8];
        unsigned dd[8];
        float dl[LM ? 8 : 1];
        [[maybe_unused]] float bg[BIAS ? 8 : 1];
        if constexpr (BIAS) {
#pragma unroll
          for (int jj = 0; jj < 8; ++jj) {
            const int sl = wslot0 + 2 * (j0 + jj);
            bg[jj] = bx.gain[bstate_s[cur][sl < nb ? sl : 0] * kBiasPitch + c];
          }
        }
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
          const int sl = wslot0 + 2 * (j0 + jj);
          info[jj] = slot_s[sl < nb ? sl : 0];
          dd[jj] = dead[sl < nb ? sl : 0];
          if constexpr (LM) dl[jj] = delta_s[cur][sl < nb ? sl : 0][c];
        }
#pragma unroll
        for (int jj = 0; jj < 8; ++jj) {
          const int sl = wslot0 + 2 * (j0 + jj);
          float child;
          if constexpr (BIAS) {
            float base = (__float_as_int(info[jj].w) == c) ? info[jj].y : info[jj].x;
            if constexpr (LM) base += lw * dl[jj];
            child = ((dd[jj] >> c) & 1u) ? -INFINITY : (base + bg[jj]) + lpc;
          } else if constexpr (LM)
            child = ((dd[jj] >> c) & 1u) ? -INFINITY : (((__float_as_int(info[jj].w) == c) ? info[jj].y : info[jj].x) + lw * dl[jj]) + lpc;
          else
            child = ((dd[jj] >> c) & 1u) ? -INFINITY : ((__float_as_int(info[jj].w) == c) ? info[jj].y : info[jj].x) + lpc;
          const float v = c == blank ? info[jj].z : child;
          ord[j0 + jj] = (sl < nb && cls_live) ? order_bits(v) : 0u;
        }
      }
#pragma unroll
      for (int j = CPL - 1; j >= 0; --j)                  // descending j + ">=": the lowest j wins a tie
        if (ord[j] >= best_ord) { best_ord = ord[j]; best_j = j; }
    }
    // (4) selection of the W best candidates, best first.
    // Fast path (threshold + rank): a cheap lower bound of the W-th largest candidate; only candidates at or above it
    // ("survivors", a few dozen) can be selected; they are compacted into LDS and every survivor finds its rank by counting
    // the survivors ahead of it (keys are unique: score, then smaller candidate index).  All of it is wave-parallel; the
    // sequential rounds below remain as the fallback for more than 128 survivors.
    int n_new = 0;
    bool selected = false;
    {
      // A lower bound of the W-th largest candidate that costs ten instructions: the lanes form 64 / 4 = 16 quads, every quad
      // maximum is a candidate, so at least 16 candidates are >= the SMALLEST quad maximum; for beams of 17 - 32 the 32 lane
      // pairs take the quads' place, for 33 - 64 the lanes themselves (round 4: those widths took the sequential path).  It
      // is looser than the W-th largest lane maximum of round 2 (flat posteriors: ~48 survivors instead of ~20 at beam 16)
      // but that bound cost a ranking of the 64 lanes -- 3 800 of the frame's 13 300 cycles as 64 v_readlane steps, 1 700 as
      // a 32-step radix select on ballots, more again as 16 four-key LDS reads -- and the survivors are ranked by counting
      // anyway; more than 128 survivors fall through to the sequential rounds.
      unsigned thr;
      if constexpr (!WIDE) {
        unsigned g = best_ord;
        if (W <= 32) g = max(g, (unsigned)dpp_i32<0xB1, 0xf, false>((int)g, (int)g));        // quad_perm [1, 0, 3, 2]: pairs
        if (W <= 16) g = max(g, (unsigned)dpp_i32<0x4E, 0xf, false>((int)g, (int)g));        // quad_perm [2, 3, 0, 1]: quads
        // (a group without a live candidate: every live candidate survives)
        thr = max(wave_min_u32(g), kOrdNegInf + 1u);
      } else {
        // beams wider than the wave: the EXACT W-th largest score, bit by bit from the top -- the largest value v with at least W
        // candidates >= v (dead candidates score 0 or order_bits(-inf): fewer than W live ones leave v below every live score)
        unsigned prefix = 0u;
        for (int bit = 31; bit >= 0; --bit) {
          const unsigned trial = prefix | (1u << bit);
          int cnt = 0;
#pragma unroll
          for (int j = 0; j < CPL; ++j) cnt += ord[j] >= trial ? 1 : 0;
          cnt = __builtin_amdgcn_readlane(wave_incl_scan_i32(cnt), 63);
          if (cnt >= W) prefix = trial;
        }
        thr = max(prefix, kOrdNegInf + 1u);
      }
      // compaction of the survivors into LDS: a lane's survivors sit behind those of the lanes below it (one wave prefix
      // sum instead of a ballot per candidate row; the keys carry the candidate index, so the order does not matter)
      int mine_n = 0;
#pragma unroll
      for (int j = 0; j < CPL; ++j) mine_n += (ord[j] >= thr && ord[j] > kOrdNegInf) ? 1 : 0;
      const int incl = wave_incl_scan_i32(mine_n);
      const int base = __builtin_amdgcn_readlane(incl, 63);
      if (base <= SURV) {
        int pos = incl - mine_n;
#pragma unroll
        for (int j = 0; j < CPL; ++j) {
          if (ord[j] >= thr && ord[j] > kOrdNegInf)
            surv[pos++] = ((unsigned long long)ord[j] << 32) | (0xFFFFFFFFu - (unsigned)(lane + 64 * j));
        }
        selected = true;
        n_new = min(base, W);
        if (lane < 16) surv[min(base + lane, SURV + 15)] = 0ull; // pad: the counting loop reads up to sixteen keys past the end
        ST_WAVE_SYNC();
        typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
        // every survivor finds its rank by counting the survivors ahead of it (keys are unique); lane l ranks survivors
        // l and l + 64
        const bool has0 = lane < base, has1 = lane + 64 < base;
        const unsigned long long mine0 = surv[has0 ? lane : 0], mine1 = surv[has1 ? lane + 64 : 0];
        int rank0 = 0, rank1 = 0;
        if constexpr (WIDE) {
          // lane l ranks survivors l, l + 64, l + 128, l + 192 against all of them, two keys per (broadcast) read
          const bool has2 = lane + 128 < base, has3 = lane + 192 < base;
          const unsigned long long mine2 = surv[has2 ? lane + 128 : 0], mine3 = surv[has3 ? lane + 192 : 0];
          int rank2 = 0, rank3 = 0;
          for (int t2 = 0; t2 < base; t2 += 2) {
            const u64x2 a = *reinterpret_cast<const u64x2*>(&surv[t2]);
            rank0 += (a[0] > mine0) + (a[1] > mine0);
            rank1 += (a[0] > mine1) + (a[1] > mine1);
            rank2 += (a[0] > mine2) + (a[1] > mine2);
            rank3 += (a[0] > mine3) + (a[1] > mine3);
          }
          if (has2 && rank2 < W) {
            sel_k[rank2] = (int)(0xFFFFFFFFu - (unsigned)mine2);
            sel_v[rank2] = order_value((unsigned)(mine2 >> 32));
          }
          if (has3 && rank3 < W) {
            sel_k[rank3] = (int)(0xFFFFFFFFu - (unsigned)mine3);
            sel_v[rank3] = order_value((unsigned)(mine3 >> 32));
          }
        } else if (base <= 64) {                                // (wave-uniform)
          // eight keys per trip, the next trip's reads issued before this trip's compares (the trip count is small and
          // every trip would otherwise wait out a full LDS round trip)
          u64x2 q[4];
#pragma unroll
          for (int k = 0; k < 4; ++k) q[k] = *reinterpret_cast<const u64x2*>(&surv[2 * k]);
          for (int t2 = 0; t2 < base; t2 += 8) {
            u64x2 n[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) n[k] = *reinterpret_cast<const u64x2*>(&surv[min(t2 + 8, SURV) + 2 * k]);
#pragma unroll
            for (int k = 0; k < 4; ++k) rank0 += (q[k][0] > mine0) + (q[k][1] > mine0);
#pragma unroll
            for (int k = 0; k < 4; ++k) q[k] = n[k];
          }
        } else {
          for (int t2 = 0; t2 < base; t2 += 4) {
            const u64x2 a = *reinterpret_cast<const u64x2*>(&surv[t2]), c2 = *reinterpret_cast<const u64x2*>(&surv[t2 + 2]);
            rank0 += (a[0] > mine0) + (a[1] > mine0) + (c2[0] > mine0) + (c2[1] > mine0);
            rank1 += (a[0] > mine1) + (a[1] > mine1) + (c2[0] > mine1) + (c2[1] > mine1);
          }
        }
        if (has0 && rank0 < W) {
          sel_k[rank0] = (int)(0xFFFFFFFFu - (unsigned)mine0);
          sel_v[rank0] = order_value((unsigned)(mine0 >> 32));
        }
        if (has1 && rank1 < W) {
          sel_k[rank1] = (int)(0xFFFFFFFFu - (unsigned)mine1);
          sel_v[rank1] = order_value((unsigned)(mine1 >> 32));
        }
      }
    }
    // Fallback: up to W rounds -- wave maximum of the scores on the DPP network, the winner is the tied lane
    // with the smallest candidate index (one lane almost always: ballot + find-first; a real tie takes a second
    // reduction); only the winner's lane retires its candidate and refreshes its local best
    for (int r = 0; !selected && r < W; ++r) {
      const unsigned top = wave_max_u32(best_ord);
      if (top <= kOrdNegInf) break;                        // nothing with non-zero probability left
      const unsigned long long tied = __ballot(best_ord == top);
      int owner = __builtin_ctzll(tied);
      if (__builtin_popcountll(tied) > 1) {
        const unsigned kmin = wave_min_u32(best_ord == top ? (unsigned)(lane + 64 * best_j) : 0xFFFFFFFFu);
        owner = (int)(kmin & 63u);
      }
      const int jw = __builtin_amdgcn_readlane(best_j, owner);
      if (lane == 0) { sel_k[r] = owner + 64 * jw; sel_v[r] = order_value(top); }
      n_new = r + 1;
      if (lane == owner) {
        best_ord = 0u;
        best_j = 0;
#pragma unroll
        for (int j = CPL - 1; j >= 0; --j) {
          if (j == jw) ord[j] = 0u;
          if (ord[j] >= best_ord) { best_ord = ord[j]; best_j = j; }
        }
      }
    }
    ST_WAVE_SYNC();
    // (5) materialise the surviving entries, best first.  Scores are kept RELATIVE to the best entry (its
    // total becomes 0) with the running offset in double: after 1500 frames the absolute log-probabilities
    // are O(-3000), where fp32 resolves only 2e-4 and near-ties at the beam boundary would be decided by
    // rounding; relative scores stay O(10) for the whole utterance.
    const float top = n_new > 0 ? sel_v[0] : 0.f;
    offset += (double)top;
#pragma unroll
    for (int e = lane; e < MAXB; e += 64) {
      if (e >= n_new) break;
      const int k = sel_k[e];
      const float v = sel_v[e];
      const int slot = WIDE ? k >> 5 : k / C, c = WIDE ? k & 31 : k - slot * C;
      // the parent entry's fields, read before the stay / child decision
      const unsigned long long h0 = S.hash[slot], ph0 = S.parent_hash[slot];
      const int len0 = S.len[slot], last0 = S.last[slot], node0 = S.node[slot];
      const float spb = stay_pb[slot], spl = stay_pl[slot];
      const bool stay = c == blank;
      const int id = 1 + (t0 + t) * W + e;
      if (!stay) nodes[id] = make_int2(node0, c);
      N.hash[e] = stay ? h0 : child_hash(h0, c);
      N.parent_hash[e] = stay ? ph0 : h0;
      N.len[e] = stay ? len0 : len0 + 1;
      N.last[e] = stay ? last0 : c;
      N.node[e] = stay ? node0 : id;
      N.pb[e] = stay ? spb - top : -INFINITY;
      N.pl[e] = stay ? spl - top : v - top;
      N.total[e] = v - top;
      if constexpr (BIAS) {
        // a child reads its state and the gain it enters with once, here; a stay keeps its parent's
        const int ps = bstate_s[cur][slot];
        const int at = ps * kBiasPitch + c;
        bstate_s[cur ^ 1][e] = stay ? ps : min(max(bx.next[at], 0), bx.n_states - 1);
        bself_s[cur ^ 1][e] = stay ? bself_s[cur][slot] : bx.gain[at];
      }
    }
    if constexpr (LM) {
      // the new entries' LM state from their parents' (all in LDS), then -- for a child -- its expansion deltas: one entry at a
      // time per lane (two unrolled would hold two sets of trie and n-gram loads in registers at once)
#pragma unroll 1
      for (int e = lane; e < n_new; e += 64) {
        const int k = sel_k[e];
        const int slot = WIDE ? k >> 5 : k / C, c = WIDE ? k & 31 : k - slot * C;
        lm_enter(lmp, lms[cur], lms[cur ^ 1], delta_s[cur][slot], delta_s[cur ^ 1][e], slot, e, c, c == blank);
      }
    }
    nb = n_new;
    cur ^= 1;
    ST_WAVE_SYNC();
  }

  __syncthreads();
  if constexpr (STREAM) {
    // the state back into the stream's record (the live set in its first buffer again); the read-out kernel does the rest
    char* rec = sx.state + b * sx.state_stride;
    copy_words(rec + kStateHeader, &sets[cur], sizeof(BeamSet<MAXB>), lane);
    if constexpr (LM) {
      copy_words(rec + kStateHeader + sizeof(BeamSet<MAXB>), &lms[cur], sizeof(LmSet<MAXB>), lane);
      copy_words(rec + kStateHeader + sizeof(BeamSet<MAXB>) + sizeof(LmSet<MAXB>), &delta_s[cur][0][0],
                 sizeof(float) * MAXB * kDeltaPitch, lane);
    }
    if constexpr (BIAS) {
      copy_words(rec + stream_state_bytes<MAXB>(LM), &bstate_s[cur][0], sizeof(int) * MAXB, lane);
      copy_words(rec + stream_state_bytes<MAXB>(LM) + sizeof(int) * MAXB, &bself_s[cur][0], sizeof(float) * MAXB, lane);
    }
    if (lane == 0) {
      hdr->magic = stream_magic(W, LM, BIAS);
      hdr->nb = nb;
      hdr->frames = t0 + Tb;
      hdr->status = status;
      if (fresh) hdr->stable_len = 0;
      hdr->pad = 0;
      hdr->offset = offset;
    }
    return;
  }
  // N best: hypothesis h is entry rank_of[h] of the final set with the total final_total[.] (both LDS, the selection's sel_k /
  // sel_v, free after the last frame); one lane per hypothesis walks its node chain -- dependent global reads, n_best chains side
  // by side, two rounds above 64 hypotheses.  Slots at or beyond the entries alive get length 0 and -inf.
  [[maybe_unused]] auto write_nbest = [&](const int* rank_of, const float* final_total) {
    if constexpr (NBEST) {
      const BeamSet<MAXB>& S = sets[cur];
      const int n = min(nx.n_best, nb);
      if (lane == 0) nx.n_hyps[ob] = n;
      for (int h = lane; h < nx.n_best; h += 64) {
        const long o = ob * nx.n_best + h;
        if (h >= n) {
          out_lens[o] = 0;
          out_logp[o] = -INFINITY;
          continue;
        }
        const int e = rank_of ? rank_of[h] : h;
        const int len = S.len[e], keep = min(len, max_out);
        out_lens[o] = len;
        out_logp[o] = (float)((double)final_total[e] + offset);
        int id = S.node[e];
        for (int i = len - 1; i >= 0; --i) {
          const int2 nd = nodes[id];
          if (i < keep) ids[o * max_out + i] = nd.y;
          id = nd.x;
        }
      }
    }
  };
  if constexpr (NBEST && !LM && !BIAS) {
    // the final set is sorted by (total desc, candidate key asc): the hypotheses are its entries 0 .. n - 1
    write_nbest(nullptr, sets[cur].total);
    return;
  }
  if constexpr (LM || BIAS) {
    // end of utterance: every entry scores its incomplete word (if non-empty) and then </s>; the top path is the best total
    // after that (ties: the lower rank).  BIAS: the open hotword match is resolved (fin: what it banks minus what it was lent).
    [[maybe_unused]] const LmSet<LMB>& L = lms[cur];
    for (int e = lane; e < nb; e += 64) {
      float v;
      if constexpr (LM) v = lm_final_total(lmp, L, delta_s[cur][e], sets[cur].total[e], e);
      else v = sets[cur].total[e];
      if constexpr (BIAS) v += bx.fin[bstate_s[cur][e]];
      sel_v[e] = v;
    }
    __syncthreads();
    if constexpr (NBEST) {
      // rank by (final total desc, rank in the set asc), by counting over LDS: entry e's place is the number of entries ahead of it
      for (int e = lane; e < nb; e += 64) {
        const float v = sel_v[e];
        int r = 0;
        for (int j = 0; j < nb; ++j) {
          const float vj = sel_v[j];
          r += (vj > v || (vj == v && j < e)) ? 1 : 0;
        }
        sel_k[r] = e;
      }
      __syncthreads();
      write_nbest(sel_k, sel_v);
      return;
    }
    if (lane == 0) {
      int e0 = 0;
      for (int e = 1; e < nb; ++e)
        if (sel_v[e] > sel_v[e0]) e0 = e;
      const BeamSet<MAXB>& S = sets[cur];
      int n = min(S.len[e0], max_out);
      out_lens[ob] = S.len[e0];
      out_logp[ob] = (float)((double)sel_v[e0] + offset);
      int id = S.node[e0];
      for (int i = S.len[e0] - 1; i >= 0; --i) {
        int2 nd = nodes[id];
        if (i < n) ids[ob * max_out + i] = nd.y;
        id = nd.x;
      }
    }
    return;
  }
  // top path: entry 0 of the final set; walk the node chain backwards
  if (lane == 0) {
    const BeamSet<MAXB>& S = sets[cur];
    int n = min(S.len[0], max_out);
    out_lens[b] = S.len[0];
    out_logp[b] = (float)((double)S.total[0] + offset);
    int id = S.node[0];
    for (int i = S.len[0] - 1; i >= 0; --i) {
      int2 nd = nodes[id];
      if (i < n) ids[(long)b * max_out + i] = nd.y;
      id = nd.x;
    }
  }
}

// ---- the stream's read-out (st_ctc_beam_stream_read) --------
// One wave per stream, on the record ctc_beam_kernel<.., STREAM> saved.  Streams without rows in this step that are neither
// finishing nor reset are skipped (their outputs stay as they are).
//  - Committed text: stable_len = the length of the longest common prefix, by LABELS, of all live entries (a prefix that left the
//    beam and came back has a second chain, so node ids say nothing).  Every future entry extends a live one, so this prefix can
//    never change.  One lane per entry (two when wide) walks its chain against entry 0's from the shortest entry's length down to
//    the stored stable_len -- never to the root -- and stops early where the two chains join.
//  - Hypothesis: open stream: entry 0 (running total).  Finishing (limit >= 0): the whole-utterance tail -- with the LM every entry
//    gains its end-of-utterance terms (lm_final_total) and the best total wins, ties to the lower rank; LM-free entry 0.
//    BIAS (a record of ctc_beam_kernel<.., STREAM, BIAS>): a finishing stream resolves every entry's open hotword match -- fin[state(e)]
//    is added after the LM's terms, with or without a model, and the best total wins as above: the tail of the biased whole-utterance
//    searches.  An open stream reports entry 0's running total, which carries the credit lent to its open match.
// result[s] = {length of the hypothesis, new stable_len, log-probability (float bits), status}; tail[s][i] = label stable_len_old + i
// of the hypothesis for i < max_tail.
//
// NBEST (ctc_beam_read_nbest_kernel, st_ctc_beam_stream_read_nbest / _step_pieces_nbest): a FINISHING read-out (limit >= 0) also writes
// the n = min(n_best, live entries) best final entries -- the list the whole-utterance N-best tail (write_nbest above) writes on the
// same rows, ranked the same way: LM-free and unbiased the set's entries 0 .. n-1, else by (fin[] desc, rank in the set asc), counted
// over LDS.  All live entries share the labels below the stored stable_len, which the host holds, so a hypothesis is its labels from
// there on, as `tail` is -- but into a compact arena instead of a fixed [n_best][max_tail] block: the wave sums its record's words,
// lane 0 reserves them with one atomicAdd on the launch's counter, and the record is written only if it lies inside the arena whole
// (the counter advances either way: it reports the demand).  Record: {stream, piece, n, old stable_len, words of the record, 0}, n
// pairs {length, log_prob bits}, the n tails back to back (length - old stable_len labels each).  One lane per hypothesis walks its
// chain, two rounds above 64.  An open stream writes nothing.  NBEST = false compiles to the read-out above (its args are empty).
template <bool NBEST>
struct ReadNbestArgs {};
template <>
struct ReadNbestArgs<true> {
  int n_best;             // 1 <= n_best <= W
  int piece;              // stamped into the header
  int* arena;             // [arena_words]
  int arena_words;
  int* used;              // the launch's counter: words asked for so far
};
constexpr int kNbestHeader = 6;

constexpr int kNoState = 2;
template <int MAXB, bool LM, bool BIAS, bool NBEST>
__device__ __forceinline__ void beam_read(const int* __restrict__ table, int W, char* __restrict__ state, long state_stride,
                                          const int2* __restrict__ node_pool, long pool_stride, int* __restrict__ tail, int max_tail,
                                          int* __restrict__ result, const LmArgs& lma, BiasArgs<BIAS> bx,
                                          const ReadNbestArgs<NBEST>& nx) {
  __shared__ float fin[MAXB];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int count = table[4 * s + 1], limit = table[4 * s + 2], reset = table[4 * s + 3];
  if (count == 0 && limit < 0 && !reset) return;
  char* rec = state + s * state_stride;
  StreamHeader* hdr = reinterpret_cast<StreamHeader*>(rec);
  int* res = result + 4 * s;
  const int nb = min(max(hdr->nb, 0), W);
  if (hdr->magic != stream_magic(W, LM, BIAS) || nb == 0) {
    if (lane == 0) {
      res[0] = 0; res[1] = 0; res[2] = __float_as_int(-INFINITY); res[3] = kNoState;
    }
    return;
  }
  const BeamSet<MAXB>& S = *reinterpret_cast<const BeamSet<MAXB>*>(rec + kStateHeader);
  const int2* __restrict__ nodes = node_pool + s * pool_stride;
  const int stable0 = hdr->stable_len;
  // the reported entry and its total
  int e0 = 0;
  float v0 = S.total[0];
  if constexpr (LM || BIAS) {
    if (limit >= 0) {
      [[maybe_unused]] const LmSet<MAXB>& L = *reinterpret_cast<const LmSet<MAXB>*>(rec + kStateHeader + sizeof(BeamSet<MAXB>));
      [[maybe_unused]] const float* deltas =
          reinterpret_cast<const float*>(rec + kStateHeader + sizeof(BeamSet<MAXB>) + sizeof(LmSet<MAXB>));
      [[maybe_unused]] const LmParams lmp{lma.v, lma.w[0][0], lma.w[0][1], lma.w[0][2], lma.oov_score};
      [[maybe_unused]] const int* bstate = reinterpret_cast<const int*>(rec + stream_state_bytes<MAXB>(LM));
      for (int e = lane; e < nb; e += 64) {
        float v;
        if constexpr (LM) v = lm_final_total(lmp, L, deltas + (long)e * kDeltaPitch, S.total[e], e);
        else v = S.total[e];
        if constexpr (BIAS) v += bx.fin[min(max(bstate[e], 0), bx.n_states - 1)];
        fin[e] = v;
      }
      __syncthreads();
      for (int e = 1; e < nb; ++e)
        if (fin[e] > fin[e0]) e0 = e;
      v0 = fin[e0];
    }
  }
  // the common prefix: no longer than the shortest live entry
  unsigned shortest = 0x7fffffffu;
#pragma unroll
  for (int e = lane; e < MAXB; e += 64)
    if (e < nb) shortest = min(shortest, (unsigned)S.len[e]);
  const int minlen = (int)wave_min_u32(shortest);
  const int len_r = S.len[0];
  int lcp = minlen;
#pragma unroll
  for (int e = lane; e < MAXB; e += 64) {
    if (e == 0 || e >= nb) continue;
    int a = S.node[e], r = S.node[0];
    for (int p = S.len[e] - 1; p >= minlen; --p) a = nodes[a].x;
    for (int p = len_r - 1; p >= minlen; --p) r = nodes[r].x;
    for (int p = minlen - 1; p >= stable0 && a != r; --p) {
      const int2 na = nodes[a], nr = nodes[r];
      if (na.y != nr.y) lcp = min(lcp, p);                       // (a lane's second entry must not raise the first one's)
      a = na.x;
      r = nr.x;
    }
  }
  const int stable = max((int)wave_min_u32((unsigned)lcp), stable0);
  // (NBEST: a finishing read-out writes `tail` in the walk of hypothesis 0 below -- the same entry, the same chain, walked once)
  const bool tail_here = !NBEST || limit < 0;
  if (lane == 0) {
    const int len0 = S.len[e0];
    int id = S.node[e0];
    for (int p = len0 - 1; tail_here && p >= stable0; --p) {
      const int2 nd = nodes[id];
      if (p - stable0 < max_tail) tail[(long)s * max_tail + (p - stable0)] = nd.y;
      id = nd.x;
    }
    res[0] = len0;
    res[1] = stable;
    res[2] = __float_as_int((float)((double)v0 + hdr->offset));
    res[3] = hdr->status;
    hdr->stable_len = stable;
  }
  if constexpr (NBEST) {
    if (limit < 0) return;                                         // (wave-uniform) an open stream has no list
    __shared__ int rank_of[MAXB];
    const int n = min(nx.n_best, nb);
    if constexpr (LM || BIAS) {
      // rank by (final total desc, rank in the set asc), by counting over LDS: entry e's place is the number of entries ahead of it
      for (int e = lane; e < nb; e += 64) {
        const float v = fin[e];
        int r = 0;
        for (int j = 0; j < nb; ++j) {
          const float vj = fin[j];
          r += (vj > v || (vj == v && j < e)) ? 1 : 0;
        }
        rank_of[r] = e;
      }
      __syncthreads();
    }
    // hypothesis h = lane + 64 k: its entry, its tail's length and the tail's place behind the pairs (a scan per round)
    constexpr int ROUNDS = MAXB / 64;
    int ent[ROUNDS], tlen[ROUNDS], toff[ROUNDS];
    int tails = 0;
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
      const int h = lane + 64 * k;
      ent[k] = 0;
      tlen[k] = 0;
      if (h < n) {
        // (hypothesis 0 is the reported entry; a NaN total would leave places of rank_of unwritten: an entry of the set either way)
        if constexpr (LM || BIAS) ent[k] = h == 0 ? e0 : min(max(rank_of[h], 0), nb - 1);
        else ent[k] = h;
        tlen[k] = max(S.len[ent[k]] - stable0, 0);
      }
      const int incl = wave_incl_scan_i32(tlen[k]);
      toff[k] = tails + incl - tlen[k];
      tails += __builtin_amdgcn_readlane(incl, 63);
    }
    const int words = kNbestHeader + 2 * n + tails;
    int base = 0;
    if (lane == 0) base = atomicAdd(nx.used, words);
    base = __builtin_amdgcn_readfirstlane(base);
    // all of the record or nothing: every index into the arena below is base + (an offset < words), and only if the record fits
    const bool fits = !(base < 0 || tails < 0 || words < 0 || (long)base + words > (long)nx.arena_words);
    int* __restrict__ rec_out = nx.arena + (fits ? base : 0);
    if (fits && lane == 0) {
      rec_out[0] = s; rec_out[1] = nx.piece; rec_out[2] = n; rec_out[3] = stable0; rec_out[4] = words; rec_out[5] = 0;
    }
    const double offset = hdr->offset;
#pragma unroll
    for (int k = 0; k < ROUNDS; ++k) {
      const int h = lane + 64 * k;
      if (h >= n || (!fits && h != 0)) continue;
      const int e = ent[k], len = S.len[e];
      float v;
      if constexpr (LM || BIAS) v = fin[e];
      else v = S.total[e];
      if (fits) {
        rec_out[kNbestHeader + 2 * h] = len;
        rec_out[kNbestHeader + 2 * h + 1] = __float_as_int((float)((double)v + offset));
      }
      int* __restrict__ out = rec_out + kNbestHeader + 2 * n + toff[k];
      int id = S.node[e];
      const int lo = len - tlen[k];                                // stable0, or len when the tail is empty
      for (int p = len - 1; p >= lo; --p) {
        const int2 nd = nodes[id];
        if (fits) out[p - lo] = nd.y;
        // hypothesis 0 is the top path (the best total, ties to the lower rank: e0 above): its labels are `tail`, fit or not
        if (h == 0 && p - lo < max_tail) tail[(long)s * max_tail + (p - lo)] = nd.y;
        id = nd.x;
      }
    }
  }
}

// the arena's counter back to 0 ahead of a call's read-outs: one more launch on the stream (a memset measured the same)
__global__ void beam_zero_word_kernel(int* __restrict__ word) {
  if (threadIdx.x == 0) *word = 0;
}

template <int MAXB, bool LM, bool BIAS = false>
__global__ __launch_bounds__(64) void ctc_beam_read_kernel(const int* __restrict__ table, int W, char* __restrict__ state, long state_stride,
                                                           const int2* __restrict__ node_pool, long pool_stride,
                                                           int* __restrict__ tail, int max_tail, int* __restrict__ result, LmArgs lma,
                                                           BiasArgs<BIAS> bx = {}) {
  beam_read<MAXB, LM, BIAS, false>(table, W, state, state_stride, node_pool, pool_stride, tail, max_tail, result, lma, bx, {});
}

template <int MAXB, bool LM, bool BIAS>
__global__ __launch_bounds__(64) void ctc_beam_read_nbest_kernel(const int* __restrict__ table, int W, char* __restrict__ state,
                                                                 long state_stride, const int2* __restrict__ node_pool, long pool_stride,
                                                                 int* __restrict__ tail, int max_tail, int* __restrict__ result, LmArgs lma,
                                                                 BiasArgs<BIAS> bx, ReadNbestArgs<true> nx) {
  beam_read<MAXB, LM, BIAS, true>(table, W, state, state_stride, node_pool, pool_stride, tail, max_tail, result, lma, bx, nx);
}

}  // namespace

extern "C" {

static size_t beam_pool_bytes(int batch, int frames, int beam_width) {
  return st::round_up((size_t)batch * ((size_t)frames * beam_width + 1) * sizeof(int2), 256);
}

// [node pool: (parent, label) pairs | log-softmax rows [batch][frames][32]]
size_t st_ctc_beam_ws(int batch, int frames, int beam_width) {
  if (batch <= 0 || frames < 0 || beam_width <= 0) return 0;
  return beam_pool_bytes(batch, frames, beam_width) + (size_t)batch * frames * kMaxClasses * sizeof(float);
}

int st_ctc_beam_search_decode(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int32_t* ids,
                              int max_out, int32_t* out_lens, float* log_prob, void* workspace,
                              size_t workspace_bytes, void* stream) {
  return st_ctc_beam_search_decode_ex(logits, seq_lens, beam_width, 0, ids, max_out, out_lens, log_prob, workspace, workspace_bytes, stream);
}

// the hotword tables of a biased search: the struct's checks (the pointers are the device's; nothing is read here)
static int bias_args(const char* who, const st_bias_tables* bias, BiasArgs<true>* bx) {
  ST_REQUIRE(bias && bias->next && bias->gain && bias->fin, "%s: null hotword tables", who);
  ST_REQUIRE(bias->n_states >= 1 && bias->n_states <= (1 << 20), "%s: hotword tables of 1..%d states supported, got %d", who, 1 << 20,
             bias->n_states);
  *bx = BiasArgs<true>{bias->next, bias->gain, bias->fin, bias->n_states};
  return ST_OK;
}

// the LM-free search: n_best = 0 is the top-path kernel of st_ctc_beam_search_decode_ex, n_best >= 1 the N-best instantiation, with
// `bias` its hotword-biased form
static int beam_search_launch(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform, int n_best,
                              int32_t* ids, int max_out, int32_t* out_lens, float* log_prob, int32_t* n_hyps, void* workspace,
                              size_t workspace_bytes, void* stream, const st_bias_tables* bias = nullptr) {
  BiasArgs<true> bx{};
  if (bias)
    if (int e = bias_args("beam search", bias, &bx)) return e;
  ST_REQUIRE(logits && logits->base && seq_lens && ids && out_lens && log_prob, "beam search: null argument");
  ST_REQUIRE(input_transform == 0 || input_transform == 1, "beam search: input_transform 0 (logits) or 1 (log10(softmax + 1e-8)), got %d",
             input_transform);
  ST_REQUIRE(logits->channels >= 2 && logits->channels <= kMaxClasses, "beam search: 2..%d classes supported, got %d",
             kMaxClasses, logits->channels);
  ST_REQUIRE(beam_width >= 1 && beam_width <= kMaxBeam, "beam search: beam width 1..%d supported, got %d", kMaxBeam,
             beam_width);
  ST_REQUIRE(max_out >= 1, "beam search: max_out must be positive");
  size_t need = st_ctc_beam_ws(logits->batch, logits->frames, beam_width);
  if (!workspace || workspace_bytes < need) {
    st::set_error("beam search: workspace of %zu bytes needed, %zu given", need, workspace_bytes);
    return ST_EWORKSPACE;
  }
  if (logits->batch == 0) return ST_OK;
  const RowMap map = st::row_map(*logits);
  float* lp_rows = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + beam_pool_bytes(logits->batch, logits->frames, beam_width));
  hipLaunchKernelGGL(logsoftmax_rows_kernel, dim3(st::ceil_div(logits->frames, 4), logits->batch), dim3(256), 0, st::as_stream(stream),
                     logits->base, map, logits->frames, logits->channels, seq_lens, input_transform, lp_rows);
  const int per_lane = st::ceil_div(beam_width * logits->channels, 64);
  if (bias)
    st::trace("ctc_beam_bias<%s> beam=%d transform=%d states=%d nbest=%d", beam_width > 64 ? "wide" : "wave", beam_width, input_transform,
              bx.n_states, n_best);
  else if (n_best > 0)
    st::trace("ctc_beam<%s> beam=%d transform=%d nbest=%d", beam_width > 64 ? "wide" : "wave", beam_width, input_transform, n_best);
  else
    st::trace("ctc_beam<%s> beam=%d transform=%d", beam_width > 64 ? "wide" : "wave", beam_width, input_transform);
#define ST_LAUNCH_BEAM_AS(CPL, MAXB, NBEST, NX)                                                                      \
  hipLaunchKernelGGL((ctc_beam_kernel<CPL, MAXB, false, NBEST>), dim3(logits->batch), dim3(64), 0, st::as_stream(stream), lp_rows, \
                     logits->frames, logits->channels, seq_lens, beam_width,                                         \
                     reinterpret_cast<int2*>(workspace), (long)logits->frames * beam_width + 1, ids, max_out,        \
                     out_lens, log_prob, LmArgs{}, NX)
#define ST_LAUNCH_BEAM_BIAS(CPL, MAXB)                                                                               \
  hipLaunchKernelGGL((ctc_beam_kernel<CPL, MAXB, false, true, false, true>), dim3(logits->batch), dim3(64), 0, st::as_stream(stream), \
                     lp_rows, logits->frames, logits->channels, seq_lens, beam_width,                                \
                     reinterpret_cast<int2*>(workspace), (long)logits->frames * beam_width + 1, ids, max_out,        \
                     out_lens, log_prob, LmArgs{}, (NbestArgs<true>{n_best, n_hyps}), StreamArgs<false>{}, bx)
#define ST_LAUNCH_BEAM(CPL, MAXB)                                                                                    \
  do {                                                                                                               \
    if (bias) ST_LAUNCH_BEAM_BIAS(CPL, MAXB);                                                                        \
    else if (n_best > 0) ST_LAUNCH_BEAM_AS(CPL, MAXB, true, (NbestArgs<true>{n_best, n_hyps}));                      \
    else ST_LAUNCH_BEAM_AS(CPL, MAXB, false, NbestArgs<false>{});                                                    \
  } while (0)
  if (beam_width > 64) ST_LAUNCH_BEAM(64, 128);
  else if (per_lane <= 4) ST_LAUNCH_BEAM(4, 64);
  else if (per_lane <= 8) ST_LAUNCH_BEAM(8, 64);
  else if (per_lane <= 16) ST_LAUNCH_BEAM(16, 64);
  else ST_LAUNCH_BEAM(32, 64);
#undef ST_LAUNCH_BEAM
#undef ST_LAUNCH_BEAM_BIAS
#undef ST_LAUNCH_BEAM_AS
  return st::check_launch("ctc_beam_search");
}

int st_ctc_beam_search_decode_ex(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform, int32_t* ids,
                                 int max_out, int32_t* out_lens, float* log_prob, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  return beam_search_launch(logits, seq_lens, beam_width, input_transform, 0, ids, max_out, out_lens, log_prob, nullptr, workspace,
                            workspace_bytes, stream);
}

int st_ctc_beam_search_decode_nbest(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform, int n_best,
                                    int32_t* ids, int max_out, int32_t* out_lens, float* log_prob, int32_t* n_hyps, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  ST_REQUIRE(n_hyps, "beam search: null argument");
  ST_REQUIRE(n_best >= 1 && n_best <= beam_width, "beam search: n_best 1..beam width (%d) supported, got %d", beam_width, n_best);
  return beam_search_launch(logits, seq_lens, beam_width, input_transform, n_best, ids, max_out, out_lens, log_prob, n_hyps, workspace,
                            workspace_bytes, stream);
}

// ... biased by hotwords (the same launch function and workspace; the top path of a biased search is its n_best = 1 list)
int st_ctc_beam_search_decode_bias_nbest(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform,
                                         const st_bias_tables* bias, int n_best, int32_t* ids, int max_out, int32_t* out_lens,
                                         float* log_prob, int32_t* n_hyps, void* workspace, size_t workspace_bytes, void* stream) {
  ST_REQUIRE(n_hyps && bias, "beam search: null argument");
  ST_REQUIRE(n_best >= 1 && n_best <= beam_width, "beam search: n_best 1..beam width (%d) supported, got %d", beam_width, n_best);
  return beam_search_launch(logits, seq_lens, beam_width, input_transform, n_best, ids, max_out, out_lens, log_prob, n_hyps, workspace,
                            workspace_bytes, stream, bias);
}

// [node pools of min(candidates, kLaunchCandidates) x batch searches | log-softmax rows [batch][frames][32]]: a launch of more
// candidates than kLaunchCandidates is split, and the launches of one call run in stream order on the same pools
size_t st_ctc_beam_lm_candidates_ws(int batch, int frames, int beam_width, int candidates) {
  if (batch <= 0 || frames < 0 || beam_width <= 0 || candidates <= 0) return 0;
  const int per_launch = candidates < kLaunchCandidates ? candidates : kLaunchCandidates;
  return beam_pool_bytes(batch * per_launch, frames, beam_width) + (size_t)batch * frames * kMaxClasses * sizeof(float);
}

// the LM-scored search for `candidates` weight triples: n_best = 0 is the top-path kernel, n_best >= 1 (one candidate) the N-best
// instantiation
static int beam_search_lm_launch(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform,
                                 void* lm, const float* weights, int candidates, float oov_score, int n_best, int32_t* ids,
                                 int max_out, int32_t* out_lens, float* log_prob, int32_t* n_hyps, void* workspace,
                                 size_t workspace_bytes, void* stream, const st_bias_tables* bias = nullptr) {
  ST_REQUIRE(logits && logits->base && seq_lens && ids && out_lens && log_prob && lm && weights, "LM beam search: null argument");
  BiasArgs<true> bx{};
  if (bias)
    if (int e = bias_args("LM beam search", bias, &bx)) return e;
  ST_REQUIRE(input_transform == 0 || input_transform == 1, "LM beam search: input_transform 0 (logits) or 1 (log10(softmax + 1e-8)), got %d",
             input_transform);
  ST_REQUIRE(logits->channels == kSpace + 2, "LM beam search: the classes must be a-z ' space blank (%d), got %d", kSpace + 2,
             logits->channels);
  ST_REQUIRE(logits->batch >= 0 && logits->frames >= 0, "LM beam search: negative batch or frames (%d, %d)", logits->batch,
             logits->frames);
  ST_REQUIRE(beam_width >= 1 && beam_width <= kMaxBeam, "LM beam search: beam width 1..%d supported, got %d", kMaxBeam, beam_width);
  ST_REQUIRE(max_out >= 1, "LM beam search: max_out must be positive");
  ST_REQUIRE(candidates >= 1, "LM beam search: candidates must be >= 1, got %d", candidates);
  ST_REQUIRE(std::isfinite(oov_score), "LM beam search: weights and oov_score must be finite");
  for (int p = 0; p < candidates; ++p)
    ST_REQUIRE(std::isfinite(weights[3 * p]) && std::isfinite(weights[3 * p + 1]) && std::isfinite(weights[3 * p + 2]),
               "LM beam search: weights and oov_score must be finite (candidate %d)", p);
  size_t need = st_ctc_beam_lm_candidates_ws(logits->batch, logits->frames, beam_width, candidates);
  if (!workspace || workspace_bytes < need) {
    st::set_error("LM beam search: workspace of %zu bytes needed, %zu given", need, workspace_bytes);
    return ST_EWORKSPACE;
  }
  // the tables' copy on the device the search runs on (a pointer into another device's memory would fault there)
  const stlm::Model* m = static_cast<const stlm::Model*>(lm);
  int device = -1;
  if (hipStreamGetDevice(st::as_stream(stream), &device) != hipSuccess) {
    st::set_error("LM beam search: hipStreamGetDevice failed");
    return ST_ELAUNCH;
  }
  const stlm::DeviceCopy* copy = m->on(device);
  ST_REQUIRE(copy, "LM beam search: the language model is not on device %d (st_lm_upload with a stream of that device)", device);
  if (logits->batch == 0) return ST_OK;
  const int per_launch = candidates < kLaunchCandidates ? candidates : kLaunchCandidates;
  const int B = logits->batch;
  const RowMap map = st::row_map(*logits);
  float* lp_rows = reinterpret_cast<float*>(reinterpret_cast<char*>(workspace) + beam_pool_bytes(B * per_launch, logits->frames, beam_width));
  // the log-softmax rows once: every candidate reads the same rows
  hipLaunchKernelGGL(logsoftmax_rows_kernel, dim3(st::ceil_div(logits->frames, 4), B), dim3(256), 0, st::as_stream(stream),
                     logits->base, map, logits->frames, logits->channels, seq_lens, input_transform, lp_rows);
  const int per_lane = st::ceil_div(beam_width * logits->channels, 64);
  if (bias)
    st::trace("ctc_beam_lm_bias<%s> beam=%d transform=%d order=%d states=%d nbest=%d", beam_width > 64 ? "wide" : "wave", beam_width,
              input_transform, copy->view.order, bx.n_states, n_best);
  else if (n_best > 0)
    st::trace("ctc_beam_lm<%s> beam=%d transform=%d order=%d candidates=%d nbest=%d", beam_width > 64 ? "wide" : "wave", beam_width,
              input_transform, copy->view.order, candidates, n_best);
  else
    st::trace("ctc_beam_lm<%s> beam=%d transform=%d order=%d candidates=%d", beam_width > 64 ? "wide" : "wave", beam_width,
              input_transform, copy->view.order, candidates);
  for (int p0 = 0; p0 < candidates; p0 += kLaunchCandidates) {
    const int n = candidates - p0 < kLaunchCandidates ? candidates - p0 : kLaunchCandidates;
    LmArgs lma{};
    lma.v = copy->view;
    lma.oov_score = oov_score;
    for (int p = 0; p < n; ++p)
      for (int k = 0; k < 3; ++k) lma.w[p][k] = weights[3 * (p0 + p) + k];
    int32_t* ids_p = ids + (size_t)p0 * B * max_out;
#define ST_LAUNCH_BEAM_AS(CPL, MAXB, NBEST, NX)                                                                      \
    hipLaunchKernelGGL((ctc_beam_kernel<CPL, MAXB, true, NBEST>), dim3(B, n), dim3(64), 0, st::as_stream(stream), lp_rows, \
                       logits->frames, logits->channels, seq_lens, beam_width,                                       \
                       reinterpret_cast<int2*>(workspace), (long)logits->frames * beam_width + 1, ids_p, max_out,    \
                       out_lens + (size_t)p0 * B, log_prob + (size_t)p0 * B, lma, NX)
#define ST_LAUNCH_BEAM_BIAS(CPL, MAXB)                                                                               \
    hipLaunchKernelGGL((ctc_beam_kernel<CPL, MAXB, true, true, false, true>), dim3(B, n), dim3(64), 0, st::as_stream(stream), lp_rows, \
                       logits->frames, logits->channels, seq_lens, beam_width,                                       \
                       reinterpret_cast<int2*>(workspace), (long)logits->frames * beam_width + 1, ids_p, max_out,    \
                       out_lens + (size_t)p0 * B, log_prob + (size_t)p0 * B, lma, (NbestArgs<true>{n_best, n_hyps}), \
                       StreamArgs<false>{}, bx)
#define ST_LAUNCH_BEAM(CPL, MAXB)                                                                                    \
    do {                                                                                                             \
      if (bias) ST_LAUNCH_BEAM_BIAS(CPL, MAXB);                                                                      \
      else if (n_best > 0) ST_LAUNCH_BEAM_AS(CPL, MAXB, true, (NbestArgs<true>{n_best, n_hyps}));                    \
      else ST_LAUNCH_BEAM_AS(CPL, MAXB, false, NbestArgs<false>{});                                                  \
    } while (0)
    if (beam_width > 64) ST_LAUNCH_BEAM(64, 128);
    else if (per_lane <= 4) ST_LAUNCH_BEAM(4, 64);
    else if (per_lane <= 8) ST_LAUNCH_BEAM(8, 64);
    else if (per_lane <= 16) ST_LAUNCH_BEAM(16, 64);
    else ST_LAUNCH_BEAM(32, 64);
#undef ST_LAUNCH_BEAM
#undef ST_LAUNCH_BEAM_BIAS
#undef ST_LAUNCH_BEAM_AS
    const int rc = st::check_launch("ctc_beam_search_lm");
    if (rc != ST_OK) return rc;
  }
  return ST_OK;
}

int st_ctc_beam_search_decode_lm_candidates(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform,
                                            void* lm, const float* weights, int candidates, float oov_score, int32_t* ids,
                                            int max_out, int32_t* out_lens, float* log_prob, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  return beam_search_lm_launch(logits, seq_lens, beam_width, input_transform, lm, weights, candidates, oov_score, 0, ids, max_out,
                               out_lens, log_prob, nullptr, workspace, workspace_bytes, stream);
}

// the single-candidate search is the candidates search with one triple (the same instantiation, the same launch shape)
int st_ctc_beam_search_decode_lm(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform, void* lm,
                                 float lm_weight, float word_count_weight, float valid_word_count_weight, float oov_score,
                                 int32_t* ids, int max_out, int32_t* out_lens, float* log_prob, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  const float w[3] = {lm_weight, word_count_weight, valid_word_count_weight};
  return st_ctc_beam_search_decode_lm_candidates(logits, seq_lens, beam_width, input_transform, lm, w, 1, oov_score, ids, max_out,
                                                 out_lens, log_prob, workspace, workspace_bytes, stream);
}

// ... and its N best final entries (one triple: the outputs are [batch][n_best])
int st_ctc_beam_search_decode_lm_nbest(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform, void* lm,
                                       float lm_weight, float word_count_weight, float valid_word_count_weight, float oov_score,
                                       int n_best, int32_t* ids, int max_out, int32_t* out_lens, float* log_prob, int32_t* n_hyps,
                                       void* workspace, size_t workspace_bytes, void* stream) {
  ST_REQUIRE(n_hyps, "LM beam search: null argument");
  ST_REQUIRE(n_best >= 1 && n_best <= beam_width, "LM beam search: n_best 1..beam width (%d) supported, got %d", beam_width, n_best);
  const float w[3] = {lm_weight, word_count_weight, valid_word_count_weight};
  return beam_search_lm_launch(logits, seq_lens, beam_width, input_transform, lm, w, 1, oov_score, n_best, ids, max_out, out_lens,
                               log_prob, n_hyps, workspace, workspace_bytes, stream);
}

// ... biased by hotwords
int st_ctc_beam_search_decode_lm_bias_nbest(const st_tensor3* logits, const int32_t* seq_lens, int beam_width, int input_transform,
                                            void* lm, float lm_weight, float word_count_weight, float valid_word_count_weight,
                                            float oov_score, const st_bias_tables* bias, int n_best, int32_t* ids, int max_out,
                                            int32_t* out_lens, float* log_prob, int32_t* n_hyps, void* workspace,
                                            size_t workspace_bytes, void* stream) {
  ST_REQUIRE(n_hyps && bias, "LM beam search: null argument");
  ST_REQUIRE(n_best >= 1 && n_best <= beam_width, "LM beam search: n_best 1..beam width (%d) supported, got %d", beam_width, n_best);
  const float w[3] = {lm_weight, word_count_weight, valid_word_count_weight};
  return beam_search_lm_launch(logits, seq_lens, beam_width, input_transform, lm, w, 1, oov_score, n_best, ids, max_out, out_lens,
                               log_prob, n_hyps, workspace, workspace_bytes, stream, bias);
}

// ---- the search carried across steps --------

size_t st_ctc_beam_stream_state_bytes(int beam_width, int lm) {
  if (beam_width < 1 || beam_width > kMaxBeam) return 0;
  return st::round_up(beam_width > 64 ? stream_state_bytes<128>(lm != 0) : stream_state_bytes<64>(lm != 0), 64);
}

// the record of a hotword-biased search: the same, then the entries' hotword states and bself (8 B per entry)
size_t st_ctc_beam_stream_bias_state_bytes(int beam_width, int lm) {
  if (beam_width < 1 || beam_width > kMaxBeam) return 0;
  return st::round_up(beam_width > 64 ? stream_bias_state_bytes<128>(lm != 0) : stream_bias_state_bytes<64>(lm != 0), 64);
}

size_t st_ctc_beam_stream_pool_bytes(int max_frames, int beam_width) {
  if (max_frames < 1 || beam_width < 1 || beam_width > kMaxBeam) return 0;
  return st::round_up(((size_t)max_frames * beam_width + 1) * sizeof(int2), 64);
}

size_t st_ctc_beam_stream_ws(int max_rows) {
  return max_rows <= 0 ? 0 : (size_t)max_rows * kMaxClasses * sizeof(float);
}

// what the two entry points share: the arguments' checks and the scorer's kernel argument (lm NULL: the LM-free search)
static int beam_stream_common(const char* who, const int32_t* table, int max_streams, int beam_width, void* lm, float lm_weight,
                              float word_count_weight, float valid_word_count_weight, float oov_score, void* state, const void* pool,
                              int max_frames, void* stream, LmArgs* lma) {
  ST_REQUIRE(table && state && pool, "%s: null argument", who);
  ST_REQUIRE(max_streams >= 1, "%s: max_streams must be positive, got %d", who, max_streams);
  ST_REQUIRE(beam_width >= 1 && beam_width <= kMaxBeam, "%s: beam width 1..%d supported, got %d", who, kMaxBeam, beam_width);
  ST_REQUIRE(max_frames >= 1 && (long)max_frames * beam_width + 1 <= 0x7fffffffL, "%s: max_frames %d with beam %d: the node ids are 31 bits",
             who, max_frames, beam_width);
  ST_REQUIRE(reinterpret_cast<uintptr_t>(state) % 8 == 0 && reinterpret_cast<uintptr_t>(pool) % 8 == 0,
             "%s: state and pool must be 8-byte aligned", who);
  *lma = LmArgs{};
  if (!lm) return ST_OK;
  ST_REQUIRE(std::isfinite(lm_weight) && std::isfinite(word_count_weight) && std::isfinite(valid_word_count_weight) &&
                 std::isfinite(oov_score), "%s: weights and oov_score must be finite", who);
  int device = -1;
  if (hipStreamGetDevice(st::as_stream(stream), &device) != hipSuccess) {
    st::set_error("%s: hipStreamGetDevice failed", who);
    return ST_ELAUNCH;
  }
  const stlm::DeviceCopy* copy = static_cast<const stlm::Model*>(lm)->on(device);
  ST_REQUIRE(copy, "%s: the language model is not on device %d (st_lm_upload with a stream of that device)", who, device);
  lma->v = copy->view;
  lma->oov_score = oov_score;
  lma->w[0][0] = lm_weight; lma->w[0][1] = word_count_weight; lma->w[0][2] = valid_word_count_weight;
  return ST_OK;
}

// the checks of a step's own arguments (st_ctc_beam_stream_step, st_ctc_beam_stream_step_pieces)
static int beam_stream_step_args(const char* who, const float* logits, int pitch, int num_classes, const int32_t* rows, int n_rows,
                                 int input_transform, void* lm) {
  ST_REQUIRE(logits && rows, "%s: null argument", who);
  ST_REQUIRE(input_transform == 0 || input_transform == 1, "%s: input_transform 0 (logits) or 1 (log10(softmax + 1e-8)), got %d", who,
             input_transform);
  if (lm)
    ST_REQUIRE(num_classes == kSpace + 2, "%s: with a language model the classes must be a-z ' space blank (%d), got %d", who, kSpace + 2,
               num_classes);
  ST_REQUIRE(num_classes >= 2 && num_classes <= kMaxClasses && pitch >= num_classes, "%s: 2..%d classes at a pitch >= classes, got %d at %d",
             who, kMaxClasses, num_classes, pitch);
  ST_REQUIRE(n_rows >= 0, "%s: negative row count %d", who, n_rows);
  return ST_OK;
}

// the hotword tables and roots of a biased stream search (bias_args' checks; `roots` is the device's, nothing is read here)
static int beam_stream_bias_args(const char* who, const st_bias_tables* bias, const int32_t* roots, BiasArgs<true, true>* sbx) {
  BiasArgs<true> bx{};
  if (int e = bias_args(who, bias, &bx)) return e;
  ST_REQUIRE(roots, "%s: null argument", who);
  *sbx = BiasArgs<true, true>{bx, roots};
  return ST_OK;
}

// one launch of the search over all streams, their work taken from `table` (device memory); sbx: the hotword-biased search
static void launch_beam_stream(const float* lp_rows, int num_classes, const int32_t* rows, const int32_t* table, int n_rows, int max_streams,
                               int beam_width, int input_transform, bool lm, const LmArgs& lma, void* state, void* pool, int max_frames,
                               hipStream_t s, const BiasArgs<true, true>* sbx = nullptr) {
  const bool wide = beam_width > 64;
  const int per_lane = st::ceil_div(beam_width * num_classes, 64);
  // (the biased lines also name the dispatch: cpl = candidates per lane of the instantiation launched)
  const int cpl = wide ? 64 : per_lane <= 4 ? 4 : per_lane <= 8 ? 8 : per_lane <= 16 ? 16 : 32;
  if (sbx && lm)
    st::trace("ctc_beam_stream_lm_bias<%s> beam=%d transform=%d order=%d states=%d streams=%d rows=%d cpl=%d", wide ? "wide" : "wave",
              beam_width, input_transform, lma.v.order, sbx->n_states, max_streams, n_rows, cpl);
  else if (sbx)
    st::trace("ctc_beam_stream_bias<%s> beam=%d transform=%d states=%d streams=%d rows=%d cpl=%d", wide ? "wide" : "wave", beam_width,
              input_transform, sbx->n_states, max_streams, n_rows, cpl);
  else if (lm)
    st::trace("ctc_beam_stream_lm<%s> beam=%d transform=%d order=%d streams=%d rows=%d", wide ? "wide" : "wave", beam_width,
              input_transform, lma.v.order, max_streams, n_rows);
  else
    st::trace("ctc_beam_stream<%s> beam=%d transform=%d streams=%d rows=%d", wide ? "wide" : "wave", beam_width, input_transform,
              max_streams, n_rows);
  const long stride = (long)(sbx ? st_ctc_beam_stream_bias_state_bytes(beam_width, lm) : st_ctc_beam_stream_state_bytes(beam_width, lm));
  const StreamArgs<true> sx{rows, table, static_cast<char*>(state), stride, max_frames};
  const long pool_stride = (long)(st_ctc_beam_stream_pool_bytes(max_frames, beam_width) / sizeof(int2));   // pairs per stream
#define ST_LAUNCH_STREAM_AS(CPL, MAXB, LM)                                                                            \
  hipLaunchKernelGGL((ctc_beam_kernel<CPL, MAXB, LM, false, true>), dim3(max_streams), dim3(64), 0, s, lp_rows, 0, num_classes, \
                     (const int*)nullptr, beam_width, reinterpret_cast<int2*>(pool), pool_stride, \
                     (int*)nullptr, 0, (int*)nullptr, (float*)nullptr, lma, NbestArgs<false>{}, sx)
#define ST_LAUNCH_STREAM_BIAS(CPL, MAXB, LM)                                                                          \
  hipLaunchKernelGGL((ctc_beam_kernel<CPL, MAXB, LM, false, true, true>), dim3(max_streams), dim3(64), 0, s, lp_rows, 0, num_classes, \
                     (const int*)nullptr, beam_width, reinterpret_cast<int2*>(pool), pool_stride, \
                     (int*)nullptr, 0, (int*)nullptr, (float*)nullptr, lma, NbestArgs<false>{}, sx, *sbx)
#define ST_LAUNCH_STREAM(CPL, MAXB)                                                                                   \
  do {                                                                                                                \
    if (sbx && lm) ST_LAUNCH_STREAM_BIAS(CPL, MAXB, true);                                                             \
    else if (sbx) ST_LAUNCH_STREAM_BIAS(CPL, MAXB, false);                                                             \
    else if (lm) ST_LAUNCH_STREAM_AS(CPL, MAXB, true);                                                                 \
    else ST_LAUNCH_STREAM_AS(CPL, MAXB, false);                                                                        \
  } while (0)
  if (cpl == 64) ST_LAUNCH_STREAM(64, 128);
  else if (cpl == 4) ST_LAUNCH_STREAM(4, 64);
  else if (cpl == 8) ST_LAUNCH_STREAM(8, 64);
  else if (cpl == 16) ST_LAUNCH_STREAM(16, 64);
  else ST_LAUNCH_STREAM(32, 64);
#undef ST_LAUNCH_STREAM
#undef ST_LAUNCH_STREAM_BIAS
#undef ST_LAUNCH_STREAM_AS
}

// one launch of the read-out over all streams
static void launch_beam_stream_read(const int32_t* table, int max_streams, int beam_width, bool lm, const LmArgs& lma, void* state,
                                    const void* pool, int max_frames, int32_t* tail, int max_tail, int32_t* result, hipStream_t s,
                                    const BiasArgs<true, true>* sbx = nullptr, const ReadNbestArgs<true>* nx = nullptr) {
  const bool wide = beam_width > 64;
  const long stride = (long)(sbx ? st_ctc_beam_stream_bias_state_bytes(beam_width, lm) : st_ctc_beam_stream_state_bytes(beam_width, lm));
  const long pool_stride = (long)(st_ctc_beam_stream_pool_bytes(max_frames, beam_width) / sizeof(int2));
  if (nx) {
    // the N-best read-out: the same eight record kinds, the unbiased ones with empty hotword arguments
    st::trace("ctc_beam_stream_read_nbest<%s%s%s> beam=%d streams=%d n_best=%d piece=%d arena=%d", wide ? "wide" : "wave", lm ? ", lm" : "",
              sbx ? ", bias" : "", beam_width, max_streams, nx->n_best, nx->piece, nx->arena_words);
#define ST_LAUNCH_READ_NBEST(MAXB, LM, BIAS, BX)                                                                      \
  hipLaunchKernelGGL((ctc_beam_read_nbest_kernel<MAXB, LM, BIAS>), dim3(max_streams), dim3(64), 0, s, table, beam_width, \
                     static_cast<char*>(state), stride, reinterpret_cast<const int2*>(pool), pool_stride, \
                     tail, max_tail, result, lma, BX, *nx)
    if (sbx) {
      const BiasArgs<true>& bx = *sbx;
      if (wide) { if (lm) ST_LAUNCH_READ_NBEST(128, true, true, bx); else ST_LAUNCH_READ_NBEST(128, false, true, bx); }
      else { if (lm) ST_LAUNCH_READ_NBEST(64, true, true, bx); else ST_LAUNCH_READ_NBEST(64, false, true, bx); }
    } else {
      const BiasArgs<false> none{};
      if (wide) { if (lm) ST_LAUNCH_READ_NBEST(128, true, false, none); else ST_LAUNCH_READ_NBEST(128, false, false, none); }
      else { if (lm) ST_LAUNCH_READ_NBEST(64, true, false, none); else ST_LAUNCH_READ_NBEST(64, false, false, none); }
    }
#undef ST_LAUNCH_READ_NBEST
    return;
  }
  st::trace("ctc_beam_stream_read<%s%s%s> beam=%d streams=%d", wide ? "wide" : "wave", lm ? ", lm" : "", sbx ? ", bias" : "", beam_width,
            max_streams);
#define ST_LAUNCH_READ(MAXB, LM)                                                                                      \
  hipLaunchKernelGGL((ctc_beam_read_kernel<MAXB, LM>), dim3(max_streams), dim3(64), 0, s, table, beam_width, \
                     static_cast<char*>(state), stride, reinterpret_cast<const int2*>(pool), pool_stride, \
                     tail, max_tail, result, lma)
#define ST_LAUNCH_READ_BIAS(MAXB, LM)                                                                                 \
  hipLaunchKernelGGL((ctc_beam_read_kernel<MAXB, LM, true>), dim3(max_streams), dim3(64), 0, s, table, beam_width, \
                     static_cast<char*>(state), stride, reinterpret_cast<const int2*>(pool), pool_stride, \
                     tail, max_tail, result, lma, static_cast<const BiasArgs<true>&>(*sbx))
  if (sbx) {
    if (wide) { if (lm) ST_LAUNCH_READ_BIAS(128, true); else ST_LAUNCH_READ_BIAS(128, false); }
    else { if (lm) ST_LAUNCH_READ_BIAS(64, true); else ST_LAUNCH_READ_BIAS(64, false); }
  } else if (wide) { if (lm) ST_LAUNCH_READ(128, true); else ST_LAUNCH_READ(128, false); }
  else { if (lm) ST_LAUNCH_READ(64, true); else ST_LAUNCH_READ(64, false); }
#undef ST_LAUNCH_READ_BIAS
#undef ST_LAUNCH_READ
}

// the list arguments of the N-best entry points (st_ctc_beam_stream_read_nbest / _step_pieces_nbest)
static int beam_stream_nbest_args(const char* who, int beam_width, const ReadNbestArgs<true>* lists) {
  ST_REQUIRE(lists->n_best >= 1 && lists->n_best <= beam_width, "%s: n_best must be 1..beam_width (%d), got %d", who, beam_width,
             lists->n_best);
  ST_REQUIRE(lists->arena && lists->used, "%s: null argument", who);
  ST_REQUIRE(lists->arena_words >= 0, "%s: negative arena_words %d", who, lists->arena_words);
  return ST_OK;
}

// the three entry points and their hotword-biased forms (`biased`: bias and roots are checked and the BIAS instantiations launched)
static int beam_stream_step(const char* who, const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table,
                            int n_rows, int max_streams, int beam_width, int input_transform, void* lm, float lm_weight,
                            float word_count_weight, float valid_word_count_weight, float oov_score, void* state, void* pool,
                            int max_frames, void* workspace, size_t workspace_bytes, void* stream, bool biased, const st_bias_tables* bias,
                            const int32_t* roots) {
  if (int e = beam_stream_step_args(who, logits, pitch, num_classes, rows, n_rows, input_transform, lm)) return e;
  LmArgs lma;
  if (int e = beam_stream_common(who, table, max_streams, beam_width, lm, lm_weight, word_count_weight, valid_word_count_weight, oov_score,
                                 state, pool, max_frames, stream, &lma))
    return e;
  BiasArgs<true, true> sbx{};
  if (biased)
    if (int e = beam_stream_bias_args(who, bias, roots, &sbx)) return e;
  const size_t need = st_ctc_beam_stream_ws(n_rows);
  if (need && (!workspace || workspace_bytes < need)) {
    st::set_error("%s: workspace of %zu bytes needed, %zu given", who, need, workspace_bytes);
    return ST_EWORKSPACE;
  }
  hipStream_t s = st::as_stream(stream);
  float* lp_rows = reinterpret_cast<float*>(workspace);
  if (n_rows > 0)
    hipLaunchKernelGGL(logsoftmax_step_rows_kernel, dim3(st::ceil_div(n_rows, 4)), dim3(256), 0, s, logits, pitch, n_rows, num_classes,
                       input_transform, lp_rows);
  launch_beam_stream(lp_rows, num_classes, rows, table, n_rows, max_streams, beam_width, input_transform, lm != nullptr, lma, state, pool,
                     max_frames, s, biased ? &sbx : nullptr);
  return st::check_launch("ctc_beam_stream_step");
}

static int beam_stream_read(const char* who, const int32_t* table, int max_streams, int beam_width, void* lm, float lm_weight,
                            float word_count_weight, float valid_word_count_weight, float oov_score, void* state, const void* pool,
                            int max_frames, int32_t* tail, int max_tail, int32_t* result, void* stream, bool biased,
                            const st_bias_tables* bias, const int32_t* roots, const ReadNbestArgs<true>* lists = nullptr) {
  ST_REQUIRE(tail && result, "%s: null argument", who);
  ST_REQUIRE(max_tail >= 1, "%s: max_tail must be positive, got %d", who, max_tail);
  LmArgs lma;
  if (int e = beam_stream_common(who, table, max_streams, beam_width, lm, lm_weight, word_count_weight, valid_word_count_weight, oov_score,
                                 state, pool, max_frames, stream, &lma))
    return e;
  BiasArgs<true, true> sbx{};
  if (biased)
    if (int e = beam_stream_bias_args(who, bias, roots, &sbx)) return e;
  if (lists) {
    if (int e = beam_stream_nbest_args(who, beam_width, lists)) return e;
    hipLaunchKernelGGL(beam_zero_word_kernel, dim3(1), dim3(64), 0, st::as_stream(stream), lists->used);
  }
  launch_beam_stream_read(table, max_streams, beam_width, lm != nullptr, lma, state, pool, max_frames, tail, max_tail, result,
                          st::as_stream(stream), biased ? &sbx : nullptr, lists);
  return st::check_launch("ctc_beam_stream_read");
}

// An endpointed step (stream_endpoint.hip wrote `pieces` [n_pieces][max_streams][4] on this stream): the log-softmax of the step's
// rows once, then for every piece in order the search and its read-out, each taking its work from pieces[p] -- device memory, so
// nothing waits for the host.  A slot {0, 0, -1, 0} makes both kernels leave at once.
static int beam_stream_step_pieces(const char* who, const float* logits, int pitch, int num_classes, const int32_t* rows,
                                   const int32_t* pieces, int n_pieces, int n_rows, int max_streams, int beam_width, int input_transform,
                                   void* lm, float lm_weight, float word_count_weight, float valid_word_count_weight, float oov_score,
                                   void* state, void* pool, int max_frames, void* workspace, size_t workspace_bytes, int32_t* tail,
                                   int max_tail, int32_t* result, void* stream, bool biased, const st_bias_tables* bias,
                                   const int32_t* roots, const ReadNbestArgs<true>* lists = nullptr) {
  if (int e = beam_stream_step_args(who, logits, pitch, num_classes, rows, n_rows, input_transform, lm)) return e;
  ST_REQUIRE(n_pieces >= 1, "%s: n_pieces must be positive, got %d", who, n_pieces);
  ST_REQUIRE(tail && result, "%s: null argument", who);
  ST_REQUIRE(max_tail >= 1, "%s: max_tail must be positive, got %d", who, max_tail);
  LmArgs lma;
  if (int e = beam_stream_common(who, pieces, max_streams, beam_width, lm, lm_weight, word_count_weight, valid_word_count_weight, oov_score,
                                 state, pool, max_frames, stream, &lma))
    return e;
  BiasArgs<true, true> sbx{};
  if (biased)
    if (int e = beam_stream_bias_args(who, bias, roots, &sbx)) return e;
  const size_t need = st_ctc_beam_stream_ws(n_rows);
  if (need && (!workspace || workspace_bytes < need)) {
    st::set_error("%s: workspace of %zu bytes needed, %zu given", who, need, workspace_bytes);
    return ST_EWORKSPACE;
  }
  if (lists)
    if (int e = beam_stream_nbest_args(who, beam_width, lists)) return e;
  hipStream_t s = st::as_stream(stream);
  if (lists) hipLaunchKernelGGL(beam_zero_word_kernel, dim3(1), dim3(64), 0, s, lists->used);
  float* lp_rows = reinterpret_cast<float*>(workspace);
  if (n_rows > 0)
    hipLaunchKernelGGL(logsoftmax_step_rows_kernel, dim3(st::ceil_div(n_rows, 4)), dim3(256), 0, s, logits, pitch, n_rows, num_classes,
                       input_transform, lp_rows);
  for (int p = 0; p < n_pieces; ++p) {
    const int32_t* table = pieces + (long)p * max_streams * 4;
    launch_beam_stream(lp_rows, num_classes, rows, table, n_rows, max_streams, beam_width, input_transform, lm != nullptr, lma, state, pool,
                       max_frames, s, biased ? &sbx : nullptr);
    ReadNbestArgs<true> piece_lists{};
    if (lists) {
      piece_lists = *lists;
      piece_lists.piece = p;
    }
    launch_beam_stream_read(table, max_streams, beam_width, lm != nullptr, lma, state, pool, max_frames,
                            tail + (long)p * max_streams * max_tail, max_tail, result + (long)p * max_streams * 4, s,
                            biased ? &sbx : nullptr, lists ? &piece_lists : nullptr);
  }
  return st::check_launch("ctc_beam_stream_step_pieces");
}

int st_ctc_beam_stream_step(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int n_rows,
                            int max_streams, int beam_width, int input_transform, void* lm, float lm_weight, float word_count_weight,
                            float valid_word_count_weight, float oov_score, void* state, void* pool, int max_frames, void* workspace,
                            size_t workspace_bytes, void* stream) {
  return beam_stream_step("beam stream step", logits, pitch, num_classes, rows, table, n_rows, max_streams, beam_width, input_transform, lm,
                          lm_weight, word_count_weight, valid_word_count_weight, oov_score, state, pool, max_frames, workspace,
                          workspace_bytes, stream, false, nullptr, nullptr);
}

int st_ctc_beam_stream_read(const int32_t* table, int max_streams, int beam_width, void* lm, float lm_weight, float word_count_weight,
                            float valid_word_count_weight, float oov_score, void* state, const void* pool, int max_frames,
                            int32_t* tail, int max_tail, int32_t* result, void* stream) {
  return beam_stream_read("beam stream read", table, max_streams, beam_width, lm, lm_weight, word_count_weight, valid_word_count_weight,
                          oov_score, state, pool, max_frames, tail, max_tail, result, stream, false, nullptr, nullptr);
}

int st_ctc_beam_stream_step_pieces(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* pieces,
                                   int n_pieces, int n_rows, int max_streams, int beam_width, int input_transform, void* lm,
                                   float lm_weight, float word_count_weight, float valid_word_count_weight, float oov_score, void* state,
                                   void* pool, int max_frames, void* workspace, size_t workspace_bytes, int32_t* tail, int max_tail,
                                   int32_t* result, void* stream) {
  return beam_stream_step_pieces("beam stream step pieces", logits, pitch, num_classes, rows, pieces, n_pieces, n_rows, max_streams,
                                 beam_width, input_transform, lm, lm_weight, word_count_weight, valid_word_count_weight, oov_score, state,
                                 pool, max_frames, workspace, workspace_bytes, tail, max_tail, result, stream, false, nullptr, nullptr);
}

// ... biased by hotwords: the records are those of st_ctc_beam_stream_bias_state_bytes, a fresh search starts in state roots[stream]
int st_ctc_beam_stream_step_bias(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* table, int n_rows,
                                 int max_streams, int beam_width, int input_transform, void* lm, float lm_weight, float word_count_weight,
                                 float valid_word_count_weight, float oov_score, void* state, void* pool, int max_frames, void* workspace,
                                 size_t workspace_bytes, void* stream, const st_bias_tables* bias, const int32_t* roots) {
  return beam_stream_step("beam stream step (hotwords)", logits, pitch, num_classes, rows, table, n_rows, max_streams, beam_width,
                          input_transform, lm, lm_weight, word_count_weight, valid_word_count_weight, oov_score, state, pool, max_frames,
                          workspace, workspace_bytes, stream, true, bias, roots);
}

int st_ctc_beam_stream_read_bias(const int32_t* table, int max_streams, int beam_width, void* lm, float lm_weight, float word_count_weight,
                                 float valid_word_count_weight, float oov_score, void* state, const void* pool, int max_frames,
                                 int32_t* tail, int max_tail, int32_t* result, void* stream, const st_bias_tables* bias,
                                 const int32_t* roots) {
  return beam_stream_read("beam stream read (hotwords)", table, max_streams, beam_width, lm, lm_weight, word_count_weight,
                          valid_word_count_weight, oov_score, state, pool, max_frames, tail, max_tail, result, stream, true, bias, roots);
}

int st_ctc_beam_stream_step_pieces_bias(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* pieces,
                                        int n_pieces, int n_rows, int max_streams, int beam_width, int input_transform, void* lm,
                                        float lm_weight, float word_count_weight, float valid_word_count_weight, float oov_score,
                                        void* state, void* pool, int max_frames, void* workspace, size_t workspace_bytes, int32_t* tail,
                                        int max_tail, int32_t* result, void* stream, const st_bias_tables* bias, const int32_t* roots) {
  return beam_stream_step_pieces("beam stream step pieces (hotwords)", logits, pitch, num_classes, rows, pieces, n_pieces, n_rows,
                                 max_streams, beam_width, input_transform, lm, lm_weight, word_count_weight, valid_word_count_weight,
                                 oov_score, state, pool, max_frames, workspace, workspace_bytes, tail, max_tail, result, stream, true, bias,
                                 roots);
}

// ... with the N-best list of every finishing read-out in a compact arena (ctc_beam_read_nbest_kernel).  bias and roots both NULL:
// the unbiased record kind.
static int nbest_kind(const char* who, const st_bias_tables* bias, const int32_t* roots, bool* biased) {
  ST_REQUIRE((bias == nullptr) == (roots == nullptr), "%s: bias and roots must be given together, or both be null", who);
  *biased = bias != nullptr;
  return ST_OK;
}

int st_ctc_beam_stream_read_nbest(const int32_t* table, int max_streams, int beam_width, void* lm, float lm_weight, float word_count_weight,
                                  float valid_word_count_weight, float oov_score, void* state, const void* pool, int max_frames,
                                  int32_t* tail, int max_tail, int32_t* result, void* stream, const st_bias_tables* bias,
                                  const int32_t* roots, int n_best, int32_t* arena, int arena_words, int32_t* arena_used) {
  const char* who = "beam stream read (N best)";
  bool biased = false;
  if (int e = nbest_kind(who, bias, roots, &biased)) return e;
  const ReadNbestArgs<true> lists{n_best, 0, arena, arena_words, arena_used};
  return beam_stream_read(who, table, max_streams, beam_width, lm, lm_weight, word_count_weight, valid_word_count_weight, oov_score, state,
                          pool, max_frames, tail, max_tail, result, stream, biased, bias, roots, &lists);
}

int st_ctc_beam_stream_step_pieces_nbest(const float* logits, int pitch, int num_classes, const int32_t* rows, const int32_t* pieces,
                                         int n_pieces, int n_rows, int max_streams, int beam_width, int input_transform, void* lm,
                                         float lm_weight, float word_count_weight, float valid_word_count_weight, float oov_score,
                                         void* state, void* pool, int max_frames, void* workspace, size_t workspace_bytes, int32_t* tail,
                                         int max_tail, int32_t* result, void* stream, const st_bias_tables* bias, const int32_t* roots,
                                         int n_best, int32_t* arena, int arena_words, int32_t* arena_used) {
  const char* who = "beam stream step pieces (N best)";
  bool biased = false;
  if (int e = nbest_kind(who, bias, roots, &biased)) return e;
  const ReadNbestArgs<true> lists{n_best, 0, arena, arena_words, arena_used};
  return beam_stream_step_pieces(who, logits, pitch, num_classes, rows, pieces, n_pieces, n_rows, max_streams, beam_width, input_transform,
                                 lm, lm_weight, word_count_weight, valid_word_count_weight, oov_score, state, pool, max_frames, workspace,
                                 workspace_bytes, tail, max_tail, result, stream, biased, bias, roots, &lists);
}

}  // extern "C"
