// dtk_engine.cpp — the run loop of a batch of rollouts, native (include/dtk.h, "dtk_engine_*").
//
// Host code only: no HIP call in this file.  The device is reached through dtk_engine_ops — for dtk_engine_create these are the
// library's own entry points (dtk_decode_batch_launch / _wait, dtk_prefill_slot, dtk_kv_fork, dtk_resume_slot, ...), for the CPU
// tests a scripted device.  What it replaces is the per-token host iteration of HF GenerationMixin._sample under
// DetikzifyGenerator.generate / rollout (reference detikzify/infer/generate.py:246-282): with 64 rollouts in one batch that loop —
// 64 Python threads woken per token behind one interpreter lock — left the GPU idle a third of the time.
//
// One thread per engine owns the context's main stream:
//   * keeps `depth` (2) steps in flight: step k+1 is queued on the device before step k's tokens are read, so the device never
//     waits for the host between steps;
//   * appends each slot's token to that slot's ring and applies the sequence's own stop rules (stop ids, token budget);
//   * wakes a slot's reader only at a flush token (a newline), after flush_max tokens, or at the end of the sequence;
//   * executes queued joins (resume in place | fork the image prefix | prefill) between steps, after the steps in flight have been
//     collected — a prefill drains the stream anyway, and a resumed slot must not be part of a step in flight.
// A text-conditioned join (dtk_engine_submit_text, the TikZero adapter) is the same join under another identity: every lookup of a
// slot's cache (resume, the prefix-cache fork) uses the pair key dtk_text_image_key(image_key, text_key), and every prefill goes
// through the text prefill, so a slot never mixes KV of the same pixels under another text (or none).
// A slot's arithmetic never depends on its company (csrc/dtk_api.hip), so which steps a sequence shares with which others —
// the only thing this loop decides differently from the Python engine it replaces — does not change a token.
#include <algorithm>
#include <array>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <deque>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dtk.h"

namespace {

using Clock = std::chrono::steady_clock;
double now_s() { return std::chrono::duration<double>(Clock::now().time_since_epoch()).count(); }

struct Seq {
  int state = 0;            // 0 = no sequence yet, else DTK_SEQ_*
  bool decoding = false;    // takes part in further steps
  std::vector<int64_t> toks;
  std::vector<float> lp, slp;       // (logprob, sample_logprob) of toks[i], kept only while a wait_lp op collects the steps (a shorter
                                    // vector = NaN for the rest: dtk_engine_read_lp)
  std::vector<int32_t> tid;         // DTK_MAX_TOP (id, logprob) entries per token, kept only while a wait_top op collects the steps (shorter
  std::vector<float> tlp;           // vectors = (-1, NaN) for the rest: dtk_engine_read_top)
  bool held = false;                // counted in the context's engine_holds (dtk_engine_create): from the join until the sequence leaves
  size_t read = 0, flushed = 0;     // toks[0, read) delivered; toks[read, flushed) may be delivered
  int budget = 0, emitted = 0;      // tokens the sequence may emit / has emitted
  int need = 0, launched = 0;       // steps to launch for it in total (budget + the forced step of a resumed slot) / launched so far
  int skip = 0;                     // 1: the next collected token is the forced last prompt token of a resumed slot (dropped)
  int n_stop = 0;
  int64_t stop[8] = {};
  int flush_mode = 0, flush_max = 64;
  int pair = -1;                    // a guided sequence (dtk_engine_submit_guided): the other slot of the pair, -1 otherwise
  bool follower = false;            // ... and this is its unconditional slot: stepped with slot `pair`, never delivered
  std::condition_variable cv;
};

struct Cmd {
  dtk_join* join = nullptr;
  dtk_join* uncond = nullptr;       // a guided sequence: the negative branch's plan, its own text and the scale
  const int64_t* utext = nullptr;
  int n_utext = 0;
  uint64_t utext_key = 0;
  float scale = 1.f;
  const int64_t* text = nullptr;    // the join's text ids (caller-owned until awaited), nullptr: an image-only join
  int n_text = 0;
  uint64_t text_key = 0;
  dtk_sampling_ext ext{};           // the sequence's min_p / epsilon_cutoff (dtk_engine_submit_ext), 0 / 0 for every other join
  float pen_p = 0.f, pen_f = 0.f;   // the sequence's presence / frequency penalty and penalty_start (dtk_engine_submit_pen), 0 / 0 / 0 for
  int pen_start = 0;                // every other join
  dtk_dry dry{0.f, 1.75f, 2, 0, 0, {}};   // the sequence's DRY (dtk_engine_submit_dry); off, at the defaults, for every other join
  dtk_length_ctl len{};             // the sequence's length rules and bias pairs (dtk_engine_submit_shape); off for every other join
  std::vector<int32_t> bias_ids;
  std::vector<float> bias_val;
  int rc = 0;
  bool done = false;
  std::condition_variable cv;
};

using ActiveSet = std::array<int32_t, DTK_MAX_BATCH>;

}  // namespace

using PrefillTextFn = int (*)(void* dev, int slot, const int64_t* ids, int T, const float* px, uint64_t image_key, const int64_t* text_ids,
                              int n_text, uint64_t text_key, int flags);
using WaitLpFn = int (*)(void* dev, int64_t* tokens_out, float* logprob_out, float* sample_logprob_out);
using WaitTopFn = int (*)(void* dev, int64_t* tokens_out, float* logprob_out, float* sample_logprob_out, int32_t* top_ids_out,
                         float* top_logprob_out);
using SamplingExtFn = int (*)(void* dev, int slot, const dtk_sampling_ext* x);
using PenaltiesFn = int (*)(void* dev, int slot, float presence, float frequency, int start);
using DryFn = int (*)(void* dev, int slot, const dtk_dry* d);
using LenFn = int (*)(void* dev, int slot, const dtk_length_ctl* l);
using BiasFn = int (*)(void* dev, int slot, const int32_t* ids, const float* values, int n);
using GuidanceFn = int (*)(void* dev, int cond_slot, int uncond_slot, float scale);
extern "C" int dtk_internal_logprobs(const dtk_ctx* c);     // dtk_api.hip, not exported: the context's "logprobs" option
extern "C" int dtk_internal_top_logprobs(const dtk_ctx* c); // ... and its "top_logprobs" (0 = off)
extern "C" void dtk_internal_engine_holds(dtk_ctx* c, int delta);   // ... which is refused while this engine holds sequences

struct dtk_engine {
  dtk_engine_ops ops{};
  PrefillTextFn prefill_text = nullptr;     // dtk_engine_set_prefill_text_op (dtk_engine_create: dtk_prefill_slot_text)
  WaitLpFn wait_lp = nullptr;               // dtk_engine_set_wait_lp_op: collects a step instead of ops.wait
  WaitTopFn wait_top = nullptr;             // dtk_engine_set_wait_top_op: collects a step instead of both (dtk_engine_create: dtk_decode_batch_wait_top)
  SamplingExtFn sampling_ext = nullptr;     // dtk_engine_set_sampling_ext_op (dtk_engine_create: dtk_set_sampling_slot_ext)
  PenaltiesFn penalties = nullptr;          // dtk_engine_set_penalties_op (dtk_engine_create: dtk_set_penalties_slot)
  DryFn dry = nullptr;                      // dtk_engine_set_dry_op (dtk_engine_create: dtk_set_dry_slot)
  LenFn length_control = nullptr;           // dtk_engine_set_length_control_op (dtk_engine_create: dtk_set_length_control_slot)
  BiasFn logit_bias = nullptr;              // dtk_engine_set_logit_bias_op (dtk_engine_create: dtk_set_logit_bias_slot)
  GuidanceFn guidance = nullptr;            // dtk_engine_set_guidance_op (dtk_engine_create: dtk_set_guidance)
  int dev_pair[DTK_MAX_BATCH];              // the pairs this engine has set on the device: the partner of a slot, -1 = none ...
  bool dev_cond[DTK_MAX_BATCH] = {};        // ... and whether the slot heads its pair (only the loop's thread touches the two)
  dtk_ctx* own_ctx = nullptr;               // dtk_engine_create: the context, whose "logprobs" option decides which wait collects
  std::mutex mu;
  std::condition_variable cv_run;
  std::condition_variable cv_idle;          // no step in flight (dtk_engine_set_option "drain")
  std::thread th;
  bool quit = false;
  std::deque<Cmd*> cmds;
  Seq seq[DTK_MAX_BATCH];
  std::deque<ActiveSet> inflight;
  int depth = 2;
  int gather_left = 0;
  Clock::time_point gather_deadline{};
  std::vector<uint8_t> flush_tok;
  dtk_engine_stats st{};
  int err_rc = 0;
  std::string err;
  double idle_from = -1.0;      // since when sequences are decoding with no step in flight (< 0: not the case)
  dtk_engine() { for (int& p : dev_pair) p = -1; }
};

namespace {

bool any_decoding(const dtk_engine* e) {
  for (const Seq& q : e->seq) if (q.decoding) return true;
  return false;
}

void mark_idle(dtk_engine* e) {
  if (e->inflight.empty() && e->idle_from < 0 && any_decoding(e)) e->idle_from = now_s();
}

// the device failed: nothing it holds can be trusted any more
void poison(dtk_engine* e, int rc) {
  if (e->err_rc) return;
  e->err_rc = rc ? rc : DTK_ERR_STATE;
  const char* t = e->ops.last_error ? e->ops.last_error(e->ops.dev) : nullptr;
  e->err = (t && *t) ? t : "device call failed";
  e->inflight.clear();
  e->cv_idle.notify_all();
  for (Seq& q : e->seq) { q.decoding = false; q.cv.notify_all(); }
}

// the loop itself found the device's results inconsistent
void poison_text(dtk_engine* e, int rc, const char* text) {
  if (e->err_rc) return;
  poison(e, rc);
  e->err = text;
}

int launch_set(dtk_engine* e, ActiveSet& set) {
  int n = 0;
  for (int s = 0; s < DTK_MAX_BATCH; ++s) {
    Seq& q = e->seq[s];
    const Seq& lead = q.follower ? e->seq[q.pair] : q;      // a pair steps together or not at all: the follower copies its leader
    set[s] = (q.decoding && lead.decoding && lead.launched < lead.need) ? 1 : 0;
    n += set[s];
  }
  return n;
}

void launch(dtk_engine* e, std::unique_lock<std::mutex>& lk, const ActiveSet& set, int n) {
  for (int s = 0; s < DTK_MAX_BATCH; ++s) if (set[s]) e->seq[s].launched++;
  const double t0 = now_s();
  if (e->inflight.empty() && e->idle_from >= 0) e->st.idle_s += t0 - e->idle_from;
  e->idle_from = -1.0;
  if (e->st.first_launch_t == 0.0) e->st.first_launch_t = t0;
  if (2 * n < e->ops.decode_slots) e->st.steps_below_half_occupancy++;
  e->inflight.push_back(set);
  lk.unlock();
  const int rc = e->ops.launch(e->ops.dev, set.data());
  const double t1 = now_s();
  lk.lock();
  e->st.launch_s += t1 - t0;
  if (rc) poison(e, rc);
}

void collect(dtk_engine* e, std::unique_lock<std::mutex>& lk, bool drain) {
  const ActiveSet set = e->inflight.front();
  int64_t toks[DTK_MAX_BATCH];
  float lp[DTK_MAX_BATCH], slp[DTK_MAX_BATCH];
  int32_t tid[DTK_MAX_BATCH * DTK_MAX_TOP];
  float tlp[DTK_MAX_BATCH * DTK_MAX_TOP];
  const WaitLpFn wait_lp = (e->own_ctx && !dtk_internal_logprobs(e->own_ctx)) ? nullptr : e->wait_lp;
  const WaitTopFn wait_top = (e->own_ctx && !dtk_internal_top_logprobs(e->own_ctx)) ? nullptr : e->wait_top;
  lk.unlock();
  const double t0 = now_s();
  const int rc = wait_top ? wait_top(e->ops.dev, toks, lp, slp, tid, tlp)
                          : wait_lp ? wait_lp(e->ops.dev, toks, lp, slp) : e->ops.wait(e->ops.dev, toks);
  const double t1 = now_s();
  lk.lock();
  if (e->err_rc) return;             // (poisoned while we waited: the queue of steps is gone)
  (drain ? e->st.drain_s : e->st.wait_s) += t1 - t0;
  if (t1 - t0 < 1e-4) e->st.host_bound_steps++;      // the device had finished already: this step waited for the host
  e->inflight.pop_front();
  if (e->inflight.empty()) e->cv_idle.notify_all();
  e->st.steps++;
  e->st.last_collect_t = t1;
  if (rc) { poison(e, rc); return; }
  for (int s = 0; s < DTK_MAX_BATCH; ++s) {
    if (!set[s]) continue;
    Seq& q = e->seq[s];
    if (q.follower) continue;                                    // handled with its leader
    Seq* f = q.pair >= 0 ? &e->seq[q.pair] : nullptr;
    if (!q.decoding) { e->st.wasted_slot_steps += f ? 2 : 1; continue; }     // ended (stop id) or left while this step was in flight (a pair: both slots)
    if (q.skip) { q.skip = 0; if (f) f->skip = 0; continue; }
    const int64_t tok = toks[s];
    if (f && toks[q.pair] != tok) {      // k_cfg_follow hands the leader's token over: anything else means the pair's caches have parted
      char text[200];
      snprintf(text, sizeof text, "guided pair (%d, %d): the unconditional slot reported token %lld, the conditional slot %lld (step %llu)",
               s, q.pair, (long long)toks[q.pair], (long long)tok, (unsigned long long)e->st.steps);
      poison_text(e, DTK_ERR_STATE, text);
      return;
    }
    q.toks.push_back(tok);
    if (wait_lp || wait_top) {      // (an op given mid-sequence: the earlier tokens' pairs are NaN)
      q.lp.resize(q.toks.size() - 1, NAN); q.slp.resize(q.toks.size() - 1, NAN);
      q.lp.push_back(lp[s]); q.slp.push_back(slp[s]);
    }
    if (wait_top) {                 // (likewise: the earlier tokens' records are (-1, NaN)).  A pair: the leader's record
      const size_t at = (q.toks.size() - 1) * DTK_MAX_TOP;
      q.tid.resize(at, -1); q.tlp.resize(at, NAN);
      q.tid.insert(q.tid.end(), tid + (size_t)s * DTK_MAX_TOP, tid + (size_t)(s + 1) * DTK_MAX_TOP);
      q.tlp.insert(q.tlp.end(), tlp + (size_t)s * DTK_MAX_TOP, tlp + (size_t)(s + 1) * DTK_MAX_TOP);
    }
    q.emitted++;
    e->st.tokens_out++;
    bool end = q.emitted >= q.budget;
    for (int k = 0; k < q.n_stop; ++k) end = end || tok == q.stop[k];
    if (end) {
      q.decoding = false;
      q.state = DTK_SEQ_FINISHED;
      q.flushed = q.toks.size();
      q.cv.notify_all();
      if (f) { f->decoding = false; f->state = DTK_SEQ_FINISHED; }
    } else if (q.flush_mode == 0 || (tok >= 0 && (size_t)tok < e->flush_tok.size() && e->flush_tok[(size_t)tok]) ||
               q.toks.size() - q.flushed >= (size_t)q.flush_max) {
      q.flushed = q.toks.size();
      q.cv.notify_all();
    }
  }
  mark_idle(e);
}

int set_error(dtk_engine* e, dtk_join* j, int rc, const char* what) {
  const char* t = e->ops.last_error ? e->ops.last_error(e->ops.dev) : nullptr;
  snprintf(j->error_out, sizeof j->error_out, "%s%s%s", what, (t && *t) ? ": " : "", (t && *t) ? t : "");
  return rc;
}

// One prompt on its way into a slot: a join, or one of the two halves of a guided sequence.  `tab` = the Cmd whose tables the slot's
// sampling gets (nullptr: neutral greedy sampling and no tables, the unconditional slot); errors are written to `err`
struct Side {
  dtk_join* j;
  const int64_t* text; int n_text; uint64_t text_key;
  const Cmd* tab;
  dtk_join* err;
};

// the identity of the slot's cache: the pair key for a text join (what dtk_prefill_slot_text stores), else the image key
uint64_t side_key(const Side& d) { return d.text ? dtk_text_image_key(d.j->image_key, d.text_key) : d.j->image_key; }

// the sequence's sampling: the plan's call, which resets min_p / epsilon_cutoff, then the join's own pair (0 / 0 without one)
int side_sampling(dtk_engine* e, const Side& d, int s) {
  const dtk_engine_ops& o = e->ops;
  dtk_join* j = d.err;
  static const Cmd neutral_tab;
  const Cmd* c = d.tab ? d.tab : &neutral_tab;
  dtk_sampling neutral{};
  neutral.temperature = 1.0f; neutral.top_p = 1.0f;
  int rc = o.set_sampling_slot(o.dev, s, d.tab ? &d.j->sampling : &neutral);
  if (rc) return set_error(e, j, rc, "dtk_set_sampling_slot");
  if (e->sampling_ext) {
    rc = e->sampling_ext(o.dev, s, &c->ext);
    if (rc) return set_error(e, j, rc, "dtk_set_sampling_slot_ext");
  }
  if (e->penalties) {       // likewise the join's own presence / frequency penalty (0 / 0 / 0 without one)
    rc = e->penalties(o.dev, s, c->pen_p, c->pen_f, c->pen_start);
    if (rc) return set_error(e, j, rc, "dtk_set_penalties_slot");
  }
  if (e->dry) {             // likewise the join's own DRY (off without one)
    rc = e->dry(o.dev, s, &c->dry);
    if (rc) return set_error(e, j, rc, "dtk_set_dry_slot");
  }
  if (e->length_control) {  // likewise the join's own length rules (off without them)
    rc = e->length_control(o.dev, s, &c->len);
    if (rc) return set_error(e, j, rc, "dtk_set_length_control_slot");
  }
  if (e->logit_bias) {      // ... and its bias pairs (none without them)
    rc = e->logit_bias(o.dev, s, c->bias_ids.data(), c->bias_val.data(), (int)c->bias_ids.size());
    if (rc) return set_error(e, j, rc, "dtk_set_logit_bias_slot");
  }
  return DTK_OK;
}

// *slot_out = the slot the join can resume in (the candidate with the longest match), -1: none
int side_can_resume(dtk_engine* e, const Side& d, int* slot_out) {
  const dtk_engine_ops& o = e->ops;
  dtk_join* j = d.j;
  *slot_out = -1;
  if (!j->try_resume || j->n_ids < 2) return DTK_OK;
  int best = -1, best_len = 0;
  const int nc = j->n_candidates > 0 ? j->n_candidates : 1;
  for (int k = 0; k < nc; ++k) {
    const int cand = j->n_candidates > 0 ? j->candidates[k] : j->slot;
    if (cand < 0 || cand >= o.decode_slots) return set_error(e, d.err, DTK_ERR_ARG, "dtk_engine_join: candidate slot out of range");
    int lcp = 0;
    const int rc = o.slot_lcp(o.dev, cand, j->ids, j->n_ids, side_key(d), &lcp);
    if (rc) return set_error(e, d.err, rc, "dtk_slot_lcp");
    if (lcp > best_len) { best = cand; best_len = lcp; }
  }
  if (best >= 0 && best_len >= j->n_ids - 1) *slot_out = best;
  return DTK_OK;
}

int side_resume(dtk_engine* e, const Side& d, int slot) {
  const dtk_engine_ops& o = e->ops;
  d.j->slot_out = slot;
  int rc = side_sampling(e, d, slot);
  if (rc) return rc;
  rc = o.resume_slot(o.dev, slot, d.j->ids, d.j->n_ids, side_key(d));
  if (rc) return set_error(e, d.err, rc, "dtk_resume_slot");
  d.j->how_out = DTK_JOIN_RESUMED;
  return DTK_OK;
}

// the join's non-resume plan: in place | fork the prefix (+ tail) | full prefill
int side_fresh(dtk_engine* e, const Side& d) {
  const dtk_engine_ops& o = e->ops;
  dtk_join* j = d.j;
  const uint64_t key = side_key(d);
  auto prefill = [&](int s, int T, int flags) {
    return d.text ? e->prefill_text(o.dev, s, j->ids, T, j->pixels, j->image_key, d.text, d.n_text, d.text_key, flags)
                  : o.prefill_slot(o.dev, s, j->ids, T, j->pixels, j->image_key, flags);
  };
  const char* prefill_name = d.text ? "dtk_prefill_slot_text" : "dtk_prefill_slot";
  const int slot = j->slot;
  j->slot_out = slot;
  int rc = side_sampling(e, d, slot);
  if (rc) return rc;
  const int reuse = DTK_PREFILL_REUSE_PREFIX | DTK_PREFILL_REUSE_IMAGE;
  if (j->prefix_len > 0 && j->prefix_in_place) {
    rc = prefill(slot, j->n_ids, reuse);
    if (rc) return set_error(e, d.err, rc, prefill_name);
    j->how_out = DTK_JOIN_IN_PLACE;
    return DTK_OK;
  }
  if (j->prefix_len > 0 && j->prefix_src >= 0) {
    if (j->prefix_len > j->n_ids) return set_error(e, d.err, DTK_ERR_ARG, "dtk_engine_join: prefix longer than the prompt");
    bool encode = j->prefix_encode != 0;
    if (!encode && j->prefix_src_whole) {
      // a prefix-cache slot the caller believes holds this prefix: check before forking its rows (a failed join may have left the
      // caller's bookkeeping behind the slot) and encode the prefix again if it does not
      int lcp = 0;
      rc = o.slot_lcp(o.dev, j->prefix_src, j->ids, j->prefix_len, key, &lcp);
      if (rc) return set_error(e, d.err, rc, "dtk_slot_lcp(prefix slot)");
      encode = lcp != j->prefix_len;
    }
    if (encode) {     // the image's first rollout: ViT + prefix prefill into the prefix-cache slot, greedy (its logits are forked)
      dtk_sampling g{};
      g.temperature = 1.0f; g.top_p = 1.0f;
      rc = o.set_sampling_slot(o.dev, j->prefix_src, &g);
      if (rc) return set_error(e, d.err, rc, "dtk_set_sampling_slot(prefix slot)");
      rc = prefill(j->prefix_src, j->prefix_len, 0);
      if (rc) return set_error(e, d.err, rc, d.text ? "dtk_prefill_slot_text(prefix slot)" : "dtk_prefill_slot(prefix slot)");
    }
    rc = o.kv_fork(o.dev, j->prefix_src, slot, j->prefix_len);
    if (rc) return set_error(e, d.err, rc, "dtk_kv_fork");
    if (j->prefix_src_whole && j->n_ids == j->prefix_len) {
      j->how_out = DTK_JOIN_FORK_WHOLE;       // KV and next-token logits came with the fork
      return DTK_OK;
    }
    rc = prefill(slot, j->n_ids, reuse);
    if (rc) return set_error(e, d.err, rc, prefill_name);
    j->how_out = DTK_JOIN_FORK_TAIL;
    return DTK_OK;
  }
  rc = prefill(slot, j->n_ids, j->full_flags);
  if (rc) return set_error(e, d.err, rc, prefill_name);
  j->how_out = DTK_JOIN_FULL;
  return DTK_OK;
}

// a pair of an earlier guided sequence still holds `slot` on the device: dissolve it before the slot gets another prompt
int dissolve_stale(dtk_engine* e, dtk_join* err, int slot) {
  const int other = e->dev_pair[slot];
  if (other < 0) return DTK_OK;
  const int cond = e->dev_cond[slot] ? slot : other;
  const int rc = e->guidance(e->ops.dev, cond, -1, 1.f);
  if (rc) return set_error(e, err, rc, "dtk_set_guidance(dissolve)");
  e->dev_pair[slot] = e->dev_pair[other] = -1;
  e->dev_cond[slot] = e->dev_cond[other] = false;
  return DTK_OK;
}

// the device side of a join; runs on the loop's thread with no step in flight and e->mu released
int do_join(dtk_engine* e, const Cmd* c) {
  dtk_join* j = c->join;
  const Side cs{j, c->text, c->n_text, c->text_key, c, j};
  j->slot_out = j->slot;
  if (!c->uncond) {
    int at = -1;
    int rc = side_can_resume(e, cs, &at);
    if (rc) return rc;
    rc = dissolve_stale(e, j, at >= 0 ? at : j->slot);
    if (rc) return rc;
    return at >= 0 ? side_resume(e, cs, at) : side_fresh(e, cs);
  }
  // a guided sequence: both prompts in, then the pair.  Nothing is paired before both halves have succeeded, and the slots' Seq records
  // are only set up after this returns DTK_OK, so a failure leaves no half-pair and both slots free
  dtk_join* u = c->uncond;
  const Side us{u, c->utext, c->n_utext, c->utext_key, nullptr, j};
  u->slot_out = u->slot;
  u->how_out = -1;
  int rc = dissolve_stale(e, j, j->slot);
  if (!rc) rc = dissolve_stale(e, j, u->slot);
  if (rc) return rc;
  int ac = -1, au = -1;
  rc = side_can_resume(e, cs, &ac);
  if (!rc) rc = side_can_resume(e, us, &au);
  if (rc) return rc;
  const bool resume = ac >= 0 && au >= 0;      // in place only if both can: the pair's slots are always in the same phase
  rc = resume ? side_resume(e, cs, ac) : side_fresh(e, cs);
  if (!rc) rc = resume ? side_resume(e, us, au) : side_fresh(e, us);
  if (rc) return rc;
  rc = e->guidance(e->ops.dev, j->slot_out, u->slot_out, c->scale);
  if (rc) return set_error(e, j, rc, "dtk_set_guidance");
  e->dev_pair[j->slot_out] = u->slot_out; e->dev_pair[u->slot_out] = j->slot_out;
  e->dev_cond[j->slot_out] = true; e->dev_cond[u->slot_out] = false;
  return DTK_OK;
}

void exec_join(dtk_engine* e, std::unique_lock<std::mutex>& lk, Cmd* c) {
  dtk_join* j = c->join;
  int rc = DTK_OK;
  j->error_out[0] = 0;
  j->slot_out = j->slot;
  j->how_out = -1;
  auto busy = [&](int s) { return s < 0 || s >= e->ops.decode_slots || s >= DTK_MAX_BATCH || e->seq[s].decoding; };
  if (e->err_rc) {
    rc = e->err_rc;
    snprintf(j->error_out, sizeof j->error_out, "the engine's device failed earlier: %s", e->err.c_str());
  } else if (!j->ids || j->n_ids < 1 || j->n_stop < 0 || j->n_stop > 8 || j->n_candidates < 0 || j->n_candidates > DTK_MAX_BATCH) {
    rc = DTK_ERR_ARG;
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_join: bad argument");
  } else if (busy(j->slot)) {
    rc = DTK_ERR_STATE;
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_join: slot %d is not a free decoding slot (0..%d)", j->slot, e->ops.decode_slots - 1);
  } else if (c->uncond && (!c->uncond->ids || c->uncond->n_ids < 1 || j->n_candidates || c->uncond->n_candidates)) {
    rc = DTK_ERR_ARG;
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_guided: bad argument (the negative branch needs ids; neither join takes candidates)");
  } else if (c->uncond && (busy(c->uncond->slot) || c->uncond->slot == j->slot)) {
    rc = DTK_ERR_STATE;
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_guided: slots %d and %d are not two free, distinct decoding slots (0..%d)", j->slot,
             c->uncond->slot, e->ops.decode_slots - 1);
  } else {
    for (int k = 0; k < j->n_candidates && !rc; ++k)
      if (busy(j->candidates[k])) {
        rc = DTK_ERR_STATE;
        snprintf(j->error_out, sizeof j->error_out, "dtk_engine_join: candidate slot %d is not a free decoding slot", j->candidates[k]);
      }
  }
  if (!rc) {
    lk.unlock();
    const double t0 = now_s();
    rc = do_join(e, c);
    const double t1 = now_s();
    lk.lock();
    e->st.join_s += t1 - t0;
    if (rc == DTK_ERR_HIP) poison(e, rc);
  }
  if (!rc) {
    // the slots' records may still name partners of earlier guided sequences (they keep them past their end, for the refusals of
    // dtk_engine_read / _leave): the new sequence starts without
    auto unlink = [&](int s) {
      Seq& o = e->seq[s];
      if (o.pair >= 0 && e->seq[o.pair].pair == s) { e->seq[o.pair].pair = -1; e->seq[o.pair].follower = false; }
      o.pair = -1; o.follower = false;
    };
    unlink(j->slot_out);
    if (c->uncond) unlink(c->uncond->slot_out);
    Seq& q = e->seq[j->slot_out];
    q.toks.clear(); q.lp.clear(); q.slp.clear(); q.tid.clear(); q.tlp.clear();
    q.read = q.flushed = 0;
    q.emitted = q.launched = 0;
    q.skip = j->how_out == DTK_JOIN_RESUMED ? 1 : 0;
    q.budget = j->max_new_tokens;
    q.pair = c->uncond ? c->uncond->slot_out : -1;
    q.follower = false;
    // never past the KV capacity: every launched step appends one position (a pair: in both slots)
    int room = e->ops.max_positions - e->ops.context_len_slot(e->ops.dev, j->slot_out);
    if (c->uncond) room = std::min(room, e->ops.max_positions - e->ops.context_len_slot(e->ops.dev, c->uncond->slot_out));
    q.need = q.budget + q.skip;
    if (q.need > room) { q.need = room > 0 ? room : 0; q.budget = q.need - q.skip; }
    q.n_stop = j->n_stop;
    for (int k = 0; k < j->n_stop; ++k) q.stop[k] = j->stop_ids[k];
    q.flush_mode = j->flush_mode;
    q.flush_max = j->flush_max > 0 ? j->flush_max : 64;
    q.decoding = q.budget > 0;
    q.state = q.decoding ? DTK_SEQ_RUNNING : DTK_SEQ_FINISHED;
    if (e->own_ctx && !q.held) { q.held = true; dtk_internal_engine_holds(e->own_ctx, +1); }
    if (c->uncond) {      // the follower: launched and stopped with its leader, nothing of it is delivered
      Seq& f = e->seq[c->uncond->slot_out];
      f.toks.clear(); f.lp.clear(); f.slp.clear(); f.tid.clear(); f.tlp.clear();
      f.read = f.flushed = 0;
      f.emitted = f.launched = 0;
      f.skip = q.skip; f.budget = q.budget; f.need = q.need; f.n_stop = 0;
      f.pair = j->slot_out; f.follower = true;
      f.decoding = q.decoding; f.state = q.state;
      if (e->own_ctx && !f.held) { f.held = true; dtk_internal_engine_holds(e->own_ctx, +1); }
    }
    e->st.joins++;
    if (q.skip) e->st.resumed++;
    if (e->gather_left > 0) e->gather_left--;
    mark_idle(e);
  }
  c->rc = rc;
  c->done = true;
  c->cv.notify_all();       // (the waiter owns `c`; it cannot run before this thread releases e->mu)
}

void run(dtk_engine* e) {
  std::unique_lock<std::mutex> lk(e->mu);
  for (;;) {
    if (e->quit) {
      while (!e->inflight.empty() && !e->err_rc) collect(e, lk, true);
      break;
    }
    if (!e->cmds.empty()) {
      while (!e->inflight.empty() && !e->err_rc) collect(e, lk, true);
      while (!e->cmds.empty()) {
        Cmd* c = e->cmds.front();
        e->cmds.pop_front();
        exec_join(e, lk, c);
      }
      continue;
    }
    if (e->err_rc) { e->cv_run.wait(lk); continue; }
    if (e->gather_left > 0 && Clock::now() >= e->gather_deadline) e->gather_left = 0;
    const bool gathering = e->gather_left > 0;
    ActiveSet set;
    const int n = gathering ? 0 : launch_set(e, set);
    if (n > 0 && (int)e->inflight.size() < e->depth) { launch(e, lk, set, n); continue; }
    if (!e->inflight.empty()) { collect(e, lk, false); continue; }
    if (gathering) e->cv_run.wait_until(lk, e->gather_deadline);
    else e->cv_run.wait(lk);
  }
}

// queue a join (text: its text ids, nullptr for an image-only join)
struct JoinPen { float presence, frequency; int start; };
struct JoinShape { const dtk_length_ctl* len; const int32_t* ids; const float* val; int n; };
inline bool len_ctl_on(const dtk_length_ctl* l) { return l && l->n_eos > 0 && (l->min_new_tokens > 0 || l->decay_factor != 0.); }
int submit(dtk_engine* e, dtk_join* j, const int64_t* text, int n_text, uint64_t text_key, uint64_t* ticket_out,
           const dtk_sampling_ext* ext = nullptr, const JoinPen* pen = nullptr, const dtk_dry* dry = nullptr,
           const JoinShape* shp = nullptr, const dtk_guided* gd = nullptr) {
  std::lock_guard<std::mutex> g(e->mu);
  if (e->quit) { snprintf(j->error_out, sizeof j->error_out, "the engine is being destroyed"); return DTK_ERR_STATE; }
  if (gd && !e->guidance) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_guided: this engine's device pairs no slots (dtk_engine_set_guidance_op)");
    return DTK_ERR_STATE;
  }
  if (gd && gd->uncond_text_ids && !e->prefill_text) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_guided: this engine's device has no text prefill (dtk_engine_set_prefill_text_op)");
    return DTK_ERR_STATE;
  }
  if (text && !e->prefill_text) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_text: this engine's device has no text prefill (dtk_engine_set_prefill_text_op)");
    return DTK_ERR_STATE;
  }
  if (ext && (ext->min_p != 0.f || ext->epsilon_cutoff != 0.f) && !e->sampling_ext) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_ext: this engine's device takes no min_p / epsilon_cutoff (dtk_engine_set_sampling_ext_op)");
    return DTK_ERR_STATE;
  }
  if (pen && (pen->presence != 0.f || pen->frequency != 0.f) && !e->penalties) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_pen: this engine's device takes no presence / frequency penalty (dtk_engine_set_penalties_op)");
    return DTK_ERR_STATE;
  }
  if (dry && dry->multiplier != 0.f && !e->dry) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_dry: this engine's device takes no DRY (dtk_engine_set_dry_op)");
    return DTK_ERR_STATE;
  }
  if (shp && len_ctl_on(shp->len) && !e->length_control) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_shape: this engine's device takes no length control (dtk_engine_set_length_control_op)");
    return DTK_ERR_STATE;
  }
  if (shp && shp->n > 0 && !e->logit_bias) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_shape: this engine's device takes no logit bias (dtk_engine_set_logit_bias_op)");
    return DTK_ERR_STATE;
  }
  Cmd* c = new Cmd();
  c->join = j;
  if (shp && shp->len) c->len = *shp->len;
  if (shp && shp->n > 0) { c->bias_ids.assign(shp->ids, shp->ids + shp->n); c->bias_val.assign(shp->val, shp->val + shp->n); }
  if (ext) c->ext = *ext;
  if (dry) c->dry = *dry;
  if (pen) { c->pen_p = pen->presence; c->pen_f = pen->frequency; c->pen_start = pen->start; }
  c->text = text; c->n_text = n_text; c->text_key = text_key;
  if (gd) { c->uncond = gd->uncond; c->utext = gd->uncond_text_ids; c->n_utext = gd->uncond_text_ids ? gd->n_uncond_text : 0; c->utext_key = gd->uncond_text_ids ? gd->uncond_text_key : 0; c->scale = gd->scale; }
  e->cmds.push_back(c);
  e->cv_run.notify_all();
  *ticket_out = (uint64_t)(uintptr_t)c;
  return DTK_OK;
}

// ---- the library's own context as the device --------------------------------------------------------------------------------------
int ctx_launch(void* d, const int32_t* a) { return dtk_decode_batch_launch((dtk_ctx*)d, a); }
int ctx_wait(void* d, int64_t* t) { return dtk_decode_batch_wait((dtk_ctx*)d, t); }
int ctx_wait_lp(void* d, int64_t* t, float* lp, float* slp) { return dtk_decode_batch_wait_lp((dtk_ctx*)d, t, lp, slp); }
int ctx_wait_top(void* d, int64_t* t, float* lp, float* slp, int32_t* ti, float* tl) { return dtk_decode_batch_wait_top((dtk_ctx*)d, t, lp, slp, ti, tl); }
int ctx_prefill(void* d, int s, const int64_t* ids, int T, const float* px, uint64_t key, int flags) { return dtk_prefill_slot((dtk_ctx*)d, s, ids, T, px, key, flags, nullptr); }
int ctx_sampling(void* d, int s, const dtk_sampling* sp) { return dtk_set_sampling_slot((dtk_ctx*)d, s, sp); }
int ctx_sampling_ext(void* d, int s, const dtk_sampling_ext* x) {     // (0 / 0: dtk_set_sampling_slot has just left exactly that)
  return (x->min_p == 0.f && x->epsilon_cutoff == 0.f) ? DTK_OK : dtk_set_sampling_slot_ext((dtk_ctx*)d, s, x);
}
int ctx_penalties(void* d, int s, float pp, float fp, int start) {     // (0 / 0: dtk_set_sampling_slot has just left exactly that)
  return (pp == 0.f && fp == 0.f) ? DTK_OK : dtk_set_penalties_slot((dtk_ctx*)d, s, pp, fp, start);
}
int ctx_dry(void* d, int s, const dtk_dry* x) {     // (off: dtk_set_sampling_slot has just left exactly that)
  return x->multiplier == 0.f ? DTK_OK : dtk_set_dry_slot((dtk_ctx*)d, s, x);
}
int ctx_length_control(void* d, int s, const dtk_length_ctl* l) {     // (off: dtk_set_sampling_slot has just left exactly that)
  return len_ctl_on(l) ? dtk_set_length_control_slot((dtk_ctx*)d, s, l) : DTK_OK;
}
int ctx_logit_bias(void* d, int s, const int32_t* ids, const float* values, int n) {
  return n > 0 ? dtk_set_logit_bias_slot((dtk_ctx*)d, s, ids, values, n) : DTK_OK;
}
int ctx_guidance(void* d, int c, int u, float g) { return dtk_set_guidance((dtk_ctx*)d, c, u, g); }
int ctx_fork(void* d, int a, int b, int n) { return dtk_kv_fork((dtk_ctx*)d, a, b, n); }
int ctx_lcp(void* d, int s, const int64_t* ids, int n, uint64_t key, int* out) { return dtk_slot_lcp((dtk_ctx*)d, s, ids, n, key, out); }
int ctx_resume(void* d, int s, const int64_t* ids, int n, uint64_t key) { return dtk_resume_slot((dtk_ctx*)d, s, ids, n, key); }
int ctx_prefill_text(void* d, int s, const int64_t* ids, int T, const float* px, uint64_t key, const int64_t* tids, int n_text, uint64_t tkey,
                     int flags) {
  return dtk_prefill_slot_text((dtk_ctx*)d, s, ids, T, px, key, tids, n_text, tkey, flags, nullptr);
}
int ctx_len(void* d, int s) { return dtk_context_len_slot((const dtk_ctx*)d, s); }
const char* ctx_err(void* d) { return dtk_last_error((const dtk_ctx*)d); }

}  // namespace

#pragma GCC visibility push(default)
extern "C" {

int dtk_engine_create_ops(const dtk_engine_ops* ops, dtk_engine** out) {
  if (!ops || !out || !ops->launch || !ops->wait || !ops->prefill_slot || !ops->set_sampling_slot || !ops->kv_fork || !ops->slot_lcp ||
      !ops->resume_slot || !ops->context_len_slot || ops->decode_slots < 1 || ops->decode_slots > DTK_MAX_BATCH || ops->max_positions < 1)
    return DTK_ERR_ARG;
  dtk_engine* e = new dtk_engine();
  e->ops = *ops;
  e->th = std::thread(run, e);
  *out = e;
  return DTK_OK;
}

int dtk_engine_create(dtk_ctx* ctx, dtk_engine** out) {
  if (!ctx || !out) return DTK_ERR_ARG;
  dtk_engine_ops o{};
  o.dev = ctx;
  o.launch = ctx_launch; o.wait = ctx_wait; o.prefill_slot = ctx_prefill; o.set_sampling_slot = ctx_sampling; o.kv_fork = ctx_fork;
  o.slot_lcp = ctx_lcp; o.resume_slot = ctx_resume; o.context_len_slot = ctx_len; o.last_error = ctx_err;
  o.max_positions = dtk_max_positions(ctx);
  o.decode_slots = dtk_max_decode_slots(ctx);
  const int rc = dtk_engine_create_ops(&o, out);
  if (rc != DTK_OK) return rc;
  {
    std::lock_guard<std::mutex> g((*out)->mu);
    (*out)->own_ctx = ctx;
    (*out)->wait_lp = ctx_wait_lp;
    (*out)->wait_top = ctx_wait_top;
    (*out)->sampling_ext = ctx_sampling_ext;
    (*out)->penalties = ctx_penalties;
    (*out)->dry = ctx_dry;
    (*out)->length_control = ctx_length_control;
    (*out)->logit_bias = ctx_logit_bias;
    (*out)->guidance = ctx_guidance;
  }
  return dtk_engine_set_prefill_text_op(*out, ctx_prefill_text);
}

int dtk_engine_set_wait_lp_op(dtk_engine* e, WaitLpFn wait_lp) {
  if (!e) return DTK_ERR_ARG;
  std::lock_guard<std::mutex> g(e->mu);
  e->wait_lp = wait_lp;
  return DTK_OK;
}

int dtk_engine_set_wait_top_op(dtk_engine* e, WaitTopFn wait_top) {
  if (!e) return DTK_ERR_ARG;
  std::lock_guard<std::mutex> g(e->mu);
  e->wait_top = wait_top;
  return DTK_OK;
}

int dtk_engine_set_sampling_ext_op(dtk_engine* e, SamplingExtFn set_sampling_slot_ext) {
  if (!e) return DTK_ERR_ARG;
  std::lock_guard<std::mutex> g(e->mu);
  e->sampling_ext = set_sampling_slot_ext;
  return DTK_OK;
}

int dtk_engine_set_penalties_op(dtk_engine* e, PenaltiesFn set_penalties_slot) {
  if (!e) return DTK_ERR_ARG;
  std::lock_guard<std::mutex> g(e->mu);
  e->penalties = set_penalties_slot;
  return DTK_OK;
}

int dtk_engine_set_dry_op(dtk_engine* e, DryFn set_dry_slot) {
  if (!e) return DTK_ERR_ARG;
  std::lock_guard<std::mutex> g(e->mu);
  e->dry = set_dry_slot;
  return DTK_OK;
}

int dtk_engine_set_length_control_op(dtk_engine* e, LenFn set_length_control_slot) {
  if (!e) return DTK_ERR_ARG;
  std::lock_guard<std::mutex> g(e->mu);
  e->length_control = set_length_control_slot;
  return DTK_OK;
}

int dtk_engine_set_logit_bias_op(dtk_engine* e, BiasFn set_logit_bias_slot) {
  if (!e) return DTK_ERR_ARG;
  std::lock_guard<std::mutex> g(e->mu);
  e->logit_bias = set_logit_bias_slot;
  return DTK_OK;
}

int dtk_engine_set_guidance_op(dtk_engine* e, GuidanceFn set_guidance) {
  if (!e) return DTK_ERR_ARG;
  std::lock_guard<std::mutex> g(e->mu);
  e->guidance = set_guidance;
  return DTK_OK;
}

int dtk_engine_set_prefill_text_op(dtk_engine* e, PrefillTextFn prefill_slot_text) {
  if (!e) return DTK_ERR_ARG;
  std::lock_guard<std::mutex> g(e->mu);
  e->prefill_text = prefill_slot_text;
  return DTK_OK;
}

void dtk_engine_destroy(dtk_engine* e) {
  if (!e) return;
  {
    std::lock_guard<std::mutex> g(e->mu);
    e->quit = true;
    e->cv_run.notify_all();
  }
  if (e->th.joinable()) e->th.join();
  {
    std::unique_lock<std::mutex> lk(e->mu);
    while (!e->cmds.empty()) {        // joins that were queued behind the stop
      Cmd* c = e->cmds.front();
      e->cmds.pop_front();
      snprintf(c->join->error_out, sizeof c->join->error_out, "the engine was destroyed");
      c->rc = DTK_ERR_STATE;
      c->done = true;
      c->cv.notify_all();
    }
    for (Seq& q : e->seq) {
      q.decoding = false;
      if (q.held) { q.held = false; dtk_internal_engine_holds(e->own_ctx, -1); }
      if (q.state == DTK_SEQ_RUNNING) q.state = DTK_SEQ_LEFT;
      q.flushed = q.toks.size();
      q.cv.notify_all();
    }
  }
  // readers that are still inside dtk_engine_read wake up under e->mu; give them the lock once more before the memory goes
  { std::lock_guard<std::mutex> g(e->mu); }
  delete e;
}

const char* dtk_engine_last_error(const dtk_engine* e) { return e ? e->err.c_str() : ""; }

int dtk_engine_set_flush_tokens(dtk_engine* e, const int64_t* ids, int n) {
  if (!e || n < 0 || (n > 0 && !ids)) return DTK_ERR_ARG;
  int64_t hi = -1;
  for (int i = 0; i < n; ++i) { if (ids[i] < 0 || ids[i] > (1 << 24)) return DTK_ERR_ARG; if (ids[i] > hi) hi = ids[i]; }
  std::lock_guard<std::mutex> g(e->mu);
  e->flush_tok.assign((size_t)(hi + 1), 0);
  for (int i = 0; i < n; ++i) e->flush_tok[(size_t)ids[i]] = 1;
  return DTK_OK;
}

int dtk_engine_set_option(dtk_engine* e, const char* name, int value) {
  if (!e || !name) return DTK_ERR_ARG;
  std::unique_lock<std::mutex> g(e->mu);
  if (!strcmp(name, "depth")) {
    if (value < 1 || value > 2) return DTK_ERR_ARG;
    e->depth = value;
    return DTK_OK;
  }
  if (!strcmp(name, "drain")) {     // block until no step is in flight (the loop collects the last steps of sequences that left on its own)
    e->cv_idle.wait(g, [&] { return e->inflight.empty() || e->err_rc != 0; });
    return DTK_OK;
  }
  return DTK_ERR_ARG;
}

int dtk_engine_expect(dtk_engine* e, int n, int timeout_ms) {
  if (!e || n < 0 || timeout_ms < 0) return DTK_ERR_ARG;
  std::lock_guard<std::mutex> g(e->mu);
  e->gather_left = n < e->ops.decode_slots ? n : e->ops.decode_slots;
  e->gather_deadline = Clock::now() + std::chrono::milliseconds(timeout_ms);
  e->st.first_launch_t = e->st.last_collect_t = 0.0;
  e->cv_run.notify_all();
  return DTK_OK;
}

int dtk_engine_submit(dtk_engine* e, dtk_join* j, uint64_t* ticket_out) {
  if (!e || !j || !ticket_out) return DTK_ERR_ARG;
  return submit(e, j, nullptr, 0, 0, ticket_out);
}

int dtk_engine_submit_text(dtk_engine* e, dtk_join* j, const int64_t* text_ids, int n_text, uint64_t text_key, uint64_t* ticket_out) {
  if (!e || !j || !ticket_out) return DTK_ERR_ARG;
  if (!text_ids || n_text < 1) { snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_text: no text"); return DTK_ERR_ARG; }
  return submit(e, j, text_ids, n_text, text_key, ticket_out);
}

int dtk_engine_submit_ext(dtk_engine* e, dtk_join* j, const dtk_sampling_ext* x, const int64_t* text_ids, int n_text, uint64_t text_key,
                          uint64_t* ticket_out) {
  if (!e || !j || !ticket_out || !x) return DTK_ERR_ARG;
  if (!(x->min_p >= 0.f && x->min_p <= 1.f) || !(x->epsilon_cutoff >= 0.f && x->epsilon_cutoff < 1.f)) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_ext: min_p must be in [0, 1] and epsilon_cutoff in [0, 1)");
    return DTK_ERR_ARG;
  }
  if (text_ids && n_text < 1) { snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_ext: no text"); return DTK_ERR_ARG; }
  return submit(e, j, text_ids, text_ids ? n_text : 0, text_ids ? text_key : 0, ticket_out, x);
}

int dtk_engine_submit_pen(dtk_engine* e, dtk_join* j, const dtk_sampling_ext* x, float presence, float frequency, int start,
                          const int64_t* text_ids, int n_text, uint64_t text_key, uint64_t* ticket_out) {
  if (!e || !j || !ticket_out) return DTK_ERR_ARG;
  if (x && (!(x->min_p >= 0.f && x->min_p <= 1.f) || !(x->epsilon_cutoff >= 0.f && x->epsilon_cutoff < 1.f))) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_pen: min_p must be in [0, 1] and epsilon_cutoff in [0, 1)");
    return DTK_ERR_ARG;
  }
  if (!(presence >= -2.f && presence <= 2.f) || !(frequency >= -2.f && frequency <= 2.f) || start < 0) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_pen: presence_penalty and frequency_penalty must be in [-2, 2], penalty_start >= 0");
    return DTK_ERR_ARG;
  }
  if (text_ids && n_text < 1) { snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_pen: no text"); return DTK_ERR_ARG; }
  const JoinPen pn{presence, frequency, start};
  return submit(e, j, text_ids, text_ids ? n_text : 0, text_ids ? text_key : 0, ticket_out, x, &pn);
}

int dtk_engine_submit_dry(dtk_engine* e, dtk_join* j, const dtk_sampling_ext* x, float presence, float frequency, int start,
                          const dtk_dry* d, const int64_t* text_ids, int n_text, uint64_t text_key, uint64_t* ticket_out) {
  if (!e || !j || !ticket_out) return DTK_ERR_ARG;
  if (x && (!(x->min_p >= 0.f && x->min_p <= 1.f) || !(x->epsilon_cutoff >= 0.f && x->epsilon_cutoff < 1.f))) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_dry: min_p must be in [0, 1] and epsilon_cutoff in [0, 1)");
    return DTK_ERR_ARG;
  }
  if (!(presence >= -2.f && presence <= 2.f) || !(frequency >= -2.f && frequency <= 2.f) || start < 0) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_dry: presence_penalty and frequency_penalty must be in [-2, 2], penalty_start >= 0");
    return DTK_ERR_ARG;
  }
  if (d && (!(d->multiplier >= 0.f && d->multiplier <= 100.f) || !(d->base >= 1.f && d->base <= 8.f) || d->allowed_length < 1 ||
            d->allowed_length > DTK_DRY_MAX_MATCH || d->start < 0 || d->n_breakers < 0 || d->n_breakers > DTK_DRY_MAX_BREAKERS)) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_dry: dry_multiplier in [0, 100], dry_base in [1, 8], dry_allowed_length in [1, 64], "
             "dry_start >= 0, at most 16 breakers");
    return DTK_ERR_ARG;
  }
  if (text_ids && n_text < 1) { snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_dry: no text"); return DTK_ERR_ARG; }
  const JoinPen pn{presence, frequency, start};
  return submit(e, j, text_ids, text_ids ? n_text : 0, text_ids ? text_key : 0, ticket_out, x, &pn, d);
}

// dtk_engine_submit_dry + the sequence's length rules and bias pairs; the values are checked here as far as they can be without the
// device (the vocabulary: an id outside it fails the join)
static int submit_shape(dtk_engine* e, dtk_join* j, const char* who, const dtk_sampling_ext* x, float presence, float frequency, int start,
                        const dtk_dry* d, const dtk_length_ctl* l, const int32_t* bias_ids, const float* bias_values, int n_bias,
                        const int64_t* text_ids, int n_text, uint64_t text_key, uint64_t* ticket_out, const dtk_guided* gd) {
  if (x && (!(x->min_p >= 0.f && x->min_p <= 1.f) || !(x->epsilon_cutoff >= 0.f && x->epsilon_cutoff < 1.f))) {
    snprintf(j->error_out, sizeof j->error_out, "%s: min_p must be in [0, 1] and epsilon_cutoff in [0, 1)", who);
    return DTK_ERR_ARG;
  }
  if (!(presence >= -2.f && presence <= 2.f) || !(frequency >= -2.f && frequency <= 2.f) || start < 0) {
    snprintf(j->error_out, sizeof j->error_out, "%s: presence_penalty and frequency_penalty must be in [-2, 2], penalty_start >= 0", who);
    return DTK_ERR_ARG;
  }
  if (d && (!(d->multiplier >= 0.f && d->multiplier <= 100.f) || !(d->base >= 1.f && d->base <= 8.f) || d->allowed_length < 1 ||
            d->allowed_length > DTK_DRY_MAX_MATCH || d->start < 0 || d->n_breakers < 0 || d->n_breakers > DTK_DRY_MAX_BREAKERS)) {
    snprintf(j->error_out, sizeof j->error_out, "%s: dry_multiplier in [0, 100], dry_base in [1, 8], dry_allowed_length in [1, 64], "
             "dry_start >= 0, at most 16 breakers", who);
    return DTK_ERR_ARG;
  }
  if (l && (l->min_new_tokens < 0 || l->decay_start < 0 || l->start < 0 || l->n_eos < 0 || l->n_eos > 8 ||
            (l->decay_factor != 0. && (!(l->decay_factor > 0. && l->decay_factor <= 1.7976931348623157e308) || l->decay_start < l->min_new_tokens)))) {
    snprintf(j->error_out, sizeof j->error_out, "%s: min_new_tokens, decay_start, length_start >= 0, decay_factor finite and > 0 "
             "(0 = none) with decay_start >= min_new_tokens, at most 8 EOS ids", who);
    return DTK_ERR_ARG;
  }
  bool bias_ok = n_bias >= 0 && n_bias <= DTK_BIAS_MAX && (n_bias == 0 || (bias_ids && bias_values));
  for (int i = 0; bias_ok && i < n_bias; ++i) bias_ok = bias_values[i] >= -100.f && bias_values[i] <= 100.f;
  if (!bias_ok) {
    snprintf(j->error_out, sizeof j->error_out, "%s: at most %d bias pairs, values finite and in [-100, 100]", who, DTK_BIAS_MAX);
    return DTK_ERR_ARG;
  }
  if (text_ids && n_text < 1) { snprintf(j->error_out, sizeof j->error_out, "%s: no text", who); return DTK_ERR_ARG; }
  const JoinPen pn{presence, frequency, start};
  const JoinShape sh{l, bias_ids, bias_values, n_bias};
  return submit(e, j, text_ids, text_ids ? n_text : 0, text_ids ? text_key : 0, ticket_out, x, &pn, d, &sh, gd);
}

int dtk_engine_submit_shape(dtk_engine* e, dtk_join* j, const dtk_sampling_ext* x, float presence, float frequency, int start,
                            const dtk_dry* d, const dtk_length_ctl* l, const int32_t* bias_ids, const float* bias_values, int n_bias,
                            const int64_t* text_ids, int n_text, uint64_t text_key, uint64_t* ticket_out) {
  if (!e || !j || !ticket_out) return DTK_ERR_ARG;
  return submit_shape(e, j, "dtk_engine_submit_shape", x, presence, frequency, start, d, l, bias_ids, bias_values, n_bias, text_ids, n_text,
                      text_key, ticket_out, nullptr);
}

// a guided sequence: dtk_engine_submit_shape for the conditional join + the negative branch's plan, its text and the scale
int dtk_engine_submit_guided(dtk_engine* e, const dtk_guided* g, const dtk_sampling_ext* x, float presence, float frequency, int start,
                             const dtk_dry* d, const dtk_length_ctl* l, const int32_t* bias_ids, const float* bias_values, int n_bias,
                             const int64_t* text_ids, int n_text, uint64_t text_key, uint64_t* ticket_out) {
  if (!e || !g || !g->cond || !g->uncond || !ticket_out) return DTK_ERR_ARG;
  dtk_join* j = g->cond;
  if (!std::isfinite(g->scale) || g->scale < 0.f || g->scale > 100.f || g->scale == 1.f) {
    snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_guided: the guidance scale must be finite, in [0, 100] and not 1");
    return DTK_ERR_ARG;
  }
  if (g->uncond_text_ids && g->n_uncond_text < 1) { snprintf(j->error_out, sizeof j->error_out, "dtk_engine_submit_guided: no negative text"); return DTK_ERR_ARG; }
  return submit_shape(e, j, "dtk_engine_submit_guided", x, presence, frequency, start, d, l, bias_ids, bias_values, n_bias, text_ids, n_text,
                      text_key, ticket_out, g);
}

int dtk_engine_await(dtk_engine* e, uint64_t ticket) {
  if (!e || !ticket) return DTK_ERR_ARG;
  Cmd* c = (Cmd*)(uintptr_t)ticket;
  int rc;
  {
    std::unique_lock<std::mutex> lk(e->mu);
    c->cv.wait(lk, [&] { return c->done; });
    rc = c->rc;
    e->cv_run.notify_all();       // a sequence may have become decodable
  }
  delete c;
  return rc;
}

int dtk_engine_join(dtk_engine* e, dtk_join* j) {
  uint64_t t = 0;
  const int rc = dtk_engine_submit(e, j, &t);
  return rc ? rc : dtk_engine_await(e, t);
}

int dtk_engine_read(dtk_engine* e, int slot, int64_t* out, int cap, int32_t* n_out, int32_t* state_out, int timeout_ms) {
  return dtk_engine_read_lp(e, slot, out, nullptr, nullptr, cap, n_out, state_out, timeout_ms);
}

int dtk_engine_read_lp(dtk_engine* e, int slot, int64_t* out, float* logprob_out, float* sample_logprob_out, int cap, int32_t* n_out,
                       int32_t* state_out, int timeout_ms) {
  return dtk_engine_read_top(e, slot, out, logprob_out, sample_logprob_out, nullptr, nullptr, cap, n_out, state_out, timeout_ms);
}

// (logprob_out == sample_logprob_out == nullptr: dtk_engine_read — the pairs are dropped; top_ids_out == top_logprob_out == nullptr:
// dtk_engine_read_lp — the records are dropped)
int dtk_engine_read_top(dtk_engine* e, int slot, int64_t* out, float* logprob_out, float* sample_logprob_out, int32_t* top_ids_out,
                        float* top_logprob_out, int cap, int32_t* n_out, int32_t* state_out, int timeout_ms) {
  if (!e || slot < 0 || slot >= DTK_MAX_BATCH || !out || cap < 1 || !n_out || !state_out || !logprob_out != !sample_logprob_out ||
      !top_ids_out != !top_logprob_out || (top_ids_out && !logprob_out))
    return DTK_ERR_ARG;
  if (logprob_out && e->own_ctx && !dtk_internal_logprobs(e->own_ctx)) return DTK_ERR_ARG;     // the context's "logprobs" option is off
  if (top_ids_out && e->own_ctx && !dtk_internal_top_logprobs(e->own_ctx)) return DTK_ERR_ARG; // ... its "top_logprobs" option
  std::unique_lock<std::mutex> lk(e->mu);
  if (top_ids_out && !e->wait_top) return DTK_ERR_ARG;      // the engine collects no records (dtk_engine_set_wait_top_op)
  Seq& q = e->seq[slot];
  if (q.follower) return DTK_ERR_ARG;      // the unconditional slot of a guided sequence: its tokens are the leader's
  *n_out = 0;
  *state_out = q.state;
  if (q.state == 0) return DTK_ERR_STATE;
  auto ready = [&] { return q.read < q.flushed || q.state != DTK_SEQ_RUNNING || e->err_rc != 0; };
  if (timeout_ms < 0) q.cv.wait(lk, ready);
  else q.cv.wait_for(lk, std::chrono::milliseconds(timeout_ms), ready);
  size_t n = q.flushed - q.read;
  if (n > (size_t)cap) n = (size_t)cap;
  if (n) memcpy(out, q.toks.data() + q.read, n * sizeof(int64_t));
  if (n && logprob_out) {
    for (size_t i = 0; i < n; ++i) {
      const size_t k = q.read + i;
      logprob_out[i] = k < q.lp.size() ? q.lp[k] : NAN;
      sample_logprob_out[i] = k < q.slp.size() ? q.slp[k] : NAN;
    }
  }
  if (n && top_ids_out) {
    for (size_t i = 0; i < n * DTK_MAX_TOP; ++i) {
      const size_t k = q.read * DTK_MAX_TOP + i;
      top_ids_out[i] = k < q.tid.size() ? q.tid[k] : -1;
      top_logprob_out[i] = k < q.tlp.size() ? q.tlp[k] : NAN;
    }
  }
  q.read += n;
  *n_out = (int32_t)n;
  if (n) e->st.reader_wakeups++;
  *state_out = (q.state != DTK_SEQ_RUNNING && q.read < q.toks.size()) ? DTK_SEQ_RUNNING : q.state;
  if (e->err_rc && n == 0 && q.state == DTK_SEQ_RUNNING) return e->err_rc;
  return DTK_OK;
}

int dtk_engine_leave(dtk_engine* e, int slot) {
  if (!e || slot < 0 || slot >= DTK_MAX_BATCH) return DTK_ERR_ARG;
  std::lock_guard<std::mutex> g(e->mu);
  Seq& q = e->seq[slot];
  if (q.follower) return DTK_ERR_ARG;      // a guided sequence leaves through its conditional slot
  if (q.pair >= 0) {                       // ... which ends both
    Seq& f = e->seq[q.pair];
    f.decoding = false;
    if (f.held) { f.held = false; dtk_internal_engine_holds(e->own_ctx, -1); }
    if (f.state == DTK_SEQ_RUNNING) f.state = DTK_SEQ_LEFT;
  }
  q.decoding = false;
  if (q.held) { q.held = false; dtk_internal_engine_holds(e->own_ctx, -1); }
  if (q.state == DTK_SEQ_RUNNING) q.state = DTK_SEQ_LEFT;
  q.flushed = q.toks.size();
  q.cv.notify_all();
  if (!any_decoding(e)) e->idle_from = -1.0;
  e->cv_run.notify_all();
  return DTK_OK;
}

int dtk_engine_get_stats(dtk_engine* e, dtk_engine_stats* out) {
  if (!e || !out) return DTK_ERR_ARG;
  std::lock_guard<std::mutex> g(e->mu);
  *out = e->st;
  return DTK_OK;
}

}  // extern "C"
#pragma GCC visibility pop
