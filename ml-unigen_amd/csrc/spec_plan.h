// The token rules of prompt-lookup speculative decoding (ug_spec_verify, text_sampler.hip) as pure functions: plain C++17, no HIP
// calls, no globals, no environment.  The kernel includes this header and applies the rules on device memory;
// tests/spec_plan_dump.cpp compiles it alone for the host and tests/test_spec_ref_cpu.py compares it with tests/spec_ref.py and with
// transformers' PromptLookupCandidateGenerator.
//
// One verify step sees the step's input tokens tok[0 .. n_draft] (tok[0] = the last emitted token, tok[1 ..] = the draft) and the
// model's greedy pick g[s] behind each of them:
//   accept   a = the number of leading s < n_draft with g[s] == tok[s + 1]
//   emit     g[0 .. a], cut after the first stop id (inclusive) and at the output width; either cut finishes the session
//   draft    on the history h[0, n): for G' = min(G, n - 1) down to 1 the smallest i with i + G' < n and h[i, i + G') == h[n - G', n)
//            (the earliest earlier occurrence of the suffix, transformers' rule); the draft is h[i + G', min(i + G' + K, n)).  The
//            first G' with a match wins; none: no draft.
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define UG_SPEC_HD __host__ __device__
#else
#define UG_SPEC_HD
#endif

namespace ug_plan {

constexpr int SPEC_MAX_ROWS = 8;          // = UG_SPEC_MAX_ROWS: 1 + the longest draft
constexpr int SPEC_MAX_NGRAM = 4;
constexpr int SPEC_MAX_STOP = 8;
constexpr int SPEC_NO_MATCH = 0x7fffffff;

// the state block of ug_spec_verify (int32, device memory; the host zeroes it at the start of a call and sets SPEC_HIST_LEN)
constexpr int SPEC_EMITTED = 0;           // tokens in out_tokens
constexpr int SPEC_DONE = 1;
constexpr int SPEC_STEPS = 2;             // verify steps that advanced the cache position
constexpr int SPEC_DRAFTED = 3;           // draft tokens those steps checked
constexpr int SPEC_ACCEPTED = 4;          // and how many of them the model agreed with
constexpr int SPEC_NDRAFT = 5;            // the draft length of the NEXT step's tok
constexpr int SPEC_HIST_LEN = 6;
constexpr int SPEC_PICK = 8;              // g[SPEC_MAX_ROWS]: the argmax launch's result
constexpr int SPEC_STATE_INTS = 16;

template <class T>
UG_SPEC_HD inline int spec_accept(const int* g, const T* tok, int n_draft) {
  int a = 0;
  while (a < n_draft && (int64_t)g[a] == (int64_t)tok[a + 1]) ++a;
  return a;
}

struct SpecEmit {
  int n;                                  // tokens emitted: g[0, n)
  int done;
};

template <class T>
UG_SPEC_HD inline SpecEmit spec_emit(const int* g, int a, const T* stop_ids, int n_stop, int emitted, int width) {
  SpecEmit e = {0, 0};
  for (int i = 0; i <= a && !e.done; ++i) {
    if (emitted + e.n >= width) break;
    ++e.n;
    for (int j = 0; j < n_stop; ++j) e.done |= (int64_t)stop_ids[j] == (int64_t)g[i];
  }
  if (emitted + e.n >= width) e.done = 1;
  return e;
}

// whether the window of g ids at i is an earlier occurrence of the last g ids of h[0, n) with at least one id behind it
UG_SPEC_HD inline bool spec_match_at(const int* h, int n, int i, int g) {
  if (i < 0 || g < 1 || i + g >= n) return false;
  for (int j = 0; j < g; ++j)
    if (h[i + j] != h[n - g + j]) return false;
  return true;
}

struct SpecDraft {
  int ngram;                              // the G' that matched (0: none)
  int start, len;                         // the draft is h[start, start + len)
};

// first[g - 1] = the smallest i with spec_match_at(h, n, i, g), SPEC_NO_MATCH without one, for g = 1 .. G  ->  the draft
UG_SPEC_HD inline SpecDraft spec_draft_from(const int* first, int n, int G, int K) {
  SpecDraft d = {0, 0, 0};
  int g = G < n - 1 ? G : n - 1;
  for (; g >= 1; --g) {
    if (first[g - 1] == SPEC_NO_MATCH) continue;
    d.ngram = g;
    d.start = first[g - 1] + g;
    d.len = n - d.start < K ? n - d.start : K;
    return d;
  }
  return d;
}

// the serial statement of the draft rule (the kernel finds `first` with all its threads instead)
UG_SPEC_HD inline SpecDraft spec_draft(const int* h, int n, int G, int K) {
  int first[SPEC_MAX_NGRAM];
  if (G > SPEC_MAX_NGRAM) G = SPEC_MAX_NGRAM;
  for (int g = 1; g <= G; ++g) {
    first[g - 1] = SPEC_NO_MATCH;
    for (int i = 0; i + g < n; ++i)
      if (spec_match_at(h, n, i, g)) { first[g - 1] = i; break; }
  }
  return spec_draft_from(first, n, G, K);
}

}  // namespace ug_plan
