// What the DOG rollout kernels share (include/muz.h, DOG rollout agent and DOG guided rollout agent): the streams of a
// rollout, the determinization of the game in LDS, the item of a phase, and the host driver of one search, which
// dog_rollout.hip (k_dog_rollout: random playouts) and dog_guided.hip (k_dog_rollout_guided: greedy-guided playouts)
// run with their own rollout kernel.
#pragma once
#include "dog_env.hpp"

namespace muz {

// Streams of a rollout (include/muz.h, DOG rollout agent).  Rollout j of the root (seed, game, turn) has its own
// 64-bit seed; the rollout's deals and random actions are the engine's own streams under that seed (dog_deal,
// random_action_uniform with the rollout's turn counter), its determinization draws the stream below.  Nothing is keyed
// by the root action: the candidates of a phase share their random numbers.
constexpr unsigned long long kDogRolloutStream = 0xD06B0110A7ull;
constexpr unsigned long long kDogRolloutMul = 0xC2B2AE3D27D4EB4Full;
constexpr unsigned long long kDogDetStream = 0xD06DE7E5ull;
constexpr unsigned long long kDogDetMul = 0x9FB21C651E98DF25ull;

__device__ __forceinline__ unsigned long long dog_rollout_seed(unsigned long long seed, int gid, int turn, int j) {
  return mix64(game_key(seed ^ kDogRolloutStream, gid, turn) ^ (unsigned long long)(j + 1) * kDogRolloutMul);
}
__device__ __forceinline__ float dog_det_uniform(unsigned long long rseed, int i) {
  return u24(mix64(rseed ^ kDogDetStream ^ (unsigned long long)(i + 1) * kDogDetMul));
}

// draw i of a determinization: the floor(u tot)-th card of the multiset in s.deck (tot > 0 cards), taken out of it
__device__ __forceinline__ int dog_det_draw(DogG& s, unsigned long long rseed, int i, int tot) {
  int k = (int)(dog_det_uniform(rseed, i) * (float)tot);
  k = k >= tot ? tot - 1 : k;
  int card = kDogCards - 1, acc = 0;
  bool found = false;
  for (int d = 0; d < kDogCards; ++d) {
    const int n = s.deck[d];
    if (!found && k < acc + n) {
      card = d;
      found = true;
    }
    acc += n;
  }
  s.deck[card] = (int8_t)(s.deck[card] - 1);
  return card;
}

// Determinization of the game in LDS (one lane).  The observers are the current player m and m' = dog_sub(m); the
// hidden multiset H is the deck plus every other seat's hand plus every other seat's swap choice (a card that left
// the hand in the swap phase and has not been handed over yet); it is gathered into s.deck.  Then, for the hidden
// seats q ascending: as many cards as q's hand held, then q's swap choice if it had one, each the floor(u |H|)-th card
// of H in card order, without replacement.  What is left of H is the deck.  Nothing else changes.
static __device__ void dog_determinize(const DetConsts& c, DogG& s, unsigned long long rseed) {
  const int m = s.cp, mp = dog_sub(c, s);
  unsigned cnt = 0u, had = 0u;   // byte q: cards in q's hand; bit q: q has a swap choice
  int tot = 0;
  for (int k = 0; k < kDogCards; ++k) tot += s.deck[k];
  for (int q = 0; q < c.P; ++q) {
    if (q == m || q == mp) continue;
    int n = 0;
    for (int k = 0; k < kDogCards; ++k) {
      const int h = s.hands[q][k];
      n += h;
      s.deck[k] = (int8_t)(s.deck[k] + h);
      s.hands[q][k] = 0;
    }
    n = n < 0 ? 0 : (n > 255 ? 255 : n);
    const int sc = s.swap_choices[q];
    if (sc >= 0 && sc < kDogCards) {
      s.deck[sc] = (int8_t)(s.deck[sc] + 1);
      had |= 1u << q;
      ++tot;
    }
    cnt |= (unsigned)n << (8 * q);
    tot += n;
  }
  int i = 0;
  for (int q = 0; q < c.P; ++q) {
    if (q == m || q == mp) continue;
    const int n = (int)((cnt >> (8 * q)) & 0xFFu);
    for (int d = 0; d < n && tot > 0; ++d) {
      const int card = dog_det_draw(s, rseed, i++, tot--);
      s.hands[q][card] = (int8_t)(s.hands[q][card] + 1);
    }
    if (((had >> q) & 1u) && tot > 0) s.swap_choices[q] = (int8_t)dog_det_draw(s, rseed, i++, tot--);
  }
}

struct DogRolloutArgs {
  DetConsts c;
  muz_dog_soa st;            // the roots (read only)
  const int32_t* game_id;    // null: the game's index
  unsigned long long seed;
  int turn, phase, R, steps, determinize;
  const int32_t* cand;       // [n][806]
  const int32_t* off;        // [n + 1] (k_dog_rollout_plan)
  int32_t* wins;             // [n][806]
  uint32_t* turns;           // [n]
  int n;
};

struct DogItem {   // the workgroup's item, in LDS (wave-uniform values re-read where they are used, not held live)
  int g, a0, gid, side;
  unsigned long long rseed;
};

// The item of a phase that k_dog_rollout and k_dog_rollout_guided play (thread 0, before the item's barrier): item i
// is candidate slot i / R of the phase's concatenated lists, rollout i % R of the phase; its game is the last g with
// off[g] <= slot (games that do not search have empty ranges).
__device__ __forceinline__ void dog_rollout_item(const DogRolloutArgs& P, int item, DogItem& it) {
  const int slot = item / P.R;
  int lo = 0, hi = P.n;   // invariant: off[lo] <= slot < off[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (P.off[mid] <= slot) lo = mid; else hi = mid;
  }
  const int gid = P.game_id ? P.game_id[lo] : lo;
  it.g = lo;
  it.a0 = P.cand[(size_t)lo * kDogActions + (slot - P.off[lo])];
  it.gid = gid;
  it.rseed = dog_rollout_seed(P.seed, gid, P.turn, P.phase * P.R + item % P.R);
}

constexpr int kRolloutGrid = 2048;   // the rollout kernels' fixed grid

// The rollout launch of one phase: `grid` workgroups of kDogPlayThreads threads on `s`.
typedef void (*DogRolloutPhase)(unsigned grid, hipStream_t s, const DogRolloutArgs& args, const void* extra);

// The host side of one search (dog_rollout.hip).  dog_rollout_check: every check of muz_dog_rollout_search, nothing
// launched; *go = false for an empty batch (MUZ_OK).  dog_rollout_launch: the candidate-list launch, then per phase
// the plan, `phase(.., extra)` and the ranking.
int dog_rollout_check(const muz_rules* rules, const muz_dog_rollout_cfg* cfg, const muz_dog_soa& st,
                      const int32_t* action, const float* value, int32_t n, const void* ws, int64_t ws_bytes,
                      DetConsts* c, bool* go);
int dog_rollout_launch(const DetConsts& c, const muz_dog_rollout_cfg* cfg, muz_dog_soa st, const int32_t* game_id,
                       int32_t* action, float* value, int32_t* visits, int32_t* wins, uint32_t* rollout_turns,
                       int32_t n, void* ws, void* stream, DogRolloutPhase phase, const void* extra);

}  // namespace muz
