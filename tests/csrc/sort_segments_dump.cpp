// CPU harness: what std::__introsort_loop LEAVES, with the sub-range every position ends in -- through the product's own serial
// pieces (radiosaber_amd/csrc/rs_sort_emul.h: median of three, unguarded partition, heap sort), in the loop's own order.
// stdin: one array per line, "n k0 k1 ... k(n-1)" (keys 0..15).  stdout per array: the n element ids (the array index each element
// started at) in the loop's order, then the n sub-range starts (a heap-sorted range: every position its own), one line.
// Checked here before anything is printed: the array equals rs_sort::introsort_loop's, and its stable sort by descending key is
// std::sort's output on the reference's element type.  Built and run by tests/test_greedy_segments_model.py.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../radiosaber_amd/csrc/rs_sort_emul.h"

typedef std::pair<std::pair<int, int>, double> elem_t;  // the reference's coord_cqi_t

static void loop_with_segments(std::vector<uint32_t>& v, std::vector<int>& seg) {
  const int n = (int)v.size();
  for (int i = 0; i < n; i++) seg[i] = 0;  // n <= 16: one sub-range
  if (n <= 1) return;
  std::vector<int> stk;
  int first = 0, last = n, depth = 2 * rs_sort::floor_log2(n);
  while (true) {
    bool heap = false;
    while (last - first > 16) {
      if (depth == 0) {
        rs_sort::heap_sort(v, first, last);
        heap = true;
        break;
      }
      --depth;
      const int mid = first + (last - first) / 2;
      rs_sort::median_to_first(v, first, first + 1, mid, last - 1);
      const int cut = rs_sort::unguarded_partition(v, first + 1, last, first);
      stk.push_back(first);
      stk.push_back(cut);
      stk.push_back(depth);
      first = cut;
    }
    for (int i = first; i < last; i++) seg[i] = heap ? i : first;
    if (stk.empty()) break;
    depth = stk.back(); stk.pop_back();
    last = stk.back(); stk.pop_back();
    first = stk.back(); stk.pop_back();
  }
}

int main() {
  const double eff[16] = {0, 0.088, 0.177, 0.311, 0.488, 0.666, 0.755, 0.977, 1.244, 1.555, 1.822, 2.088, 2.444, 2.888, 3.244, 3.955};
  int n;
  while (scanf("%d", &n) == 1) {
    std::vector<int> keys(n);
    for (int i = 0; i < n; i++)
      if (scanf("%d", &keys[i]) != 1 || keys[i] < 0 || keys[i] > 15) return 2;
    std::vector<uint32_t> v(n), w(n);
    for (int i = 0; i < n; i++) v[i] = w[i] = ((uint32_t)keys[i] << 16) | (uint32_t)i;
    std::vector<int> seg(n), stk(3 * 64);
    loop_with_segments(v, seg);
    rs_sort::introsort_loop(w, n, stk);
    if (v != w) { fprintf(stderr, "the loop with sub-ranges and rs_sort::introsort_loop disagree\n"); return 1; }
    std::vector<elem_t> ref(n);
    for (int i = 0; i < n; i++) ref[i] = elem_t(std::make_pair(i, 0), eff[keys[i]]);
    std::sort(ref.begin(), ref.end(), [](elem_t a, elem_t b) { return a.second > b.second; });
    std::stable_sort(w.begin(), w.end(), [](uint32_t a, uint32_t b) { return (a >> 16) > (b >> 16); });
    for (int i = 0; i < n; i++)
      if ((int)(w[i] & 0xFFFF) != ref[i].first.first) { fprintf(stderr, "std::sort disagrees at %d\n", i); return 1; }
    for (int i = 0; i < n; i++) printf("%d ", (int)(v[i] & 0xFFFF));
    for (int i = 0; i < n; i++) printf("%d ", seg[i]);
    printf("\n");
  }
  return 0;
}
