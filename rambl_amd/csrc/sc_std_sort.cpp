// std::sort as libstdc++ permutes it (GCC <bits/stl_algo.h>: introsort with
// median-of-three to first, unguarded partition, heap fallback, final insertion
// sort with threshold 16).  See sc_std_sort.hpp.
#include "sc_std_sort.hpp"
#include <algorithm>

namespace sc {

namespace {
struct Sorter {
    std::vector<int>& a;
    const std::function<bool(int, int)>& less;
    void linear_insert(int last) {
        int val = a[last];
        int next = last - 1;
        while (less(val, a[next])) { a[last] = a[next]; last = next; --next; }
        a[last] = val;
    }
    void insertion(int first, int last) {
        if (first == last) return;
        for (int i = first + 1; i != last; ++i) {
            if (less(a[i], a[first])) {
                int val = a[i];
                std::move_backward(a.begin() + first, a.begin() + i, a.begin() + i + 1);
                a[first] = val;
            } else linear_insert(i);
        }
    }
    void push_heap(int first, int hole, int top, int value) {
        int parent = (hole - 1) / 2;
        while (hole > top && less(a[first + parent], value)) {
            a[first + hole] = a[first + parent];
            hole = parent;
            parent = (hole - 1) / 2;
        }
        a[first + hole] = value;
    }
    void adjust_heap(int first, int hole, int len, int value) {
        const int top = hole;
        int child = hole;
        while (child < (len - 1) / 2) {
            child = 2 * (child + 1);
            if (less(a[first + child], a[first + child - 1])) child--;
            a[first + hole] = a[first + child];
            hole = child;
        }
        if ((len & 1) == 0 && child == (len - 2) / 2) {
            child = 2 * (child + 1);
            a[first + hole] = a[first + child - 1];
            hole = child - 1;
        }
        push_heap(first, hole, top, value);
    }
    void heap_sort(int first, int last) {
        int len = last - first;
        if (len >= 2) {
            int parent = (len - 2) / 2;
            for (;;) {
                int value = a[first + parent];
                adjust_heap(first, parent, len, value);
                if (parent == 0) break;
                parent--;
            }
        }
        while (last - first > 1) {
            --last;
            int value = a[last];
            a[last] = a[first];
            adjust_heap(first, 0, last - first, value);
        }
    }
    void median_to_first(int result, int x, int y, int z) {
        if (less(a[x], a[y])) {
            if (less(a[y], a[z])) std::swap(a[result], a[y]);
            else if (less(a[x], a[z])) std::swap(a[result], a[z]);
            else std::swap(a[result], a[x]);
        } else if (less(a[x], a[z])) std::swap(a[result], a[x]);
        else if (less(a[y], a[z])) std::swap(a[result], a[z]);
        else std::swap(a[result], a[y]);
    }
    int partition(int first, int last, int pivot) {
        for (;;) {
            while (less(a[first], a[pivot])) ++first;
            --last;
            while (less(a[pivot], a[last])) --last;
            if (!(first < last)) return first;
            std::swap(a[first], a[last]);
            ++first;
        }
    }
    void introsort(int first, int last, int depth) {
        while (last - first > 16) {
            if (depth == 0) { heap_sort(first, last); return; }
            --depth;
            int mid = first + (last - first) / 2;
            median_to_first(first, first + 1, mid, last - 1);
            int cut = partition(first + 1, last, first);
            introsort(cut, last, depth);
            last = cut;
        }
    }
};
}  // namespace

void std_sort_perm(std::vector<int>& idx, const std::function<bool(int, int)>& less) {
    int n = (int)idx.size();
    if (n == 0) return;
    Sorter s{idx, less};
    int lg = 0;
    for (unsigned t = (unsigned)n; t > 1; t >>= 1) lg++;
    s.introsort(0, n, lg * 2);
    if (n > 16) {
        s.insertion(0, 16);
        for (int i = 16; i != n; ++i) s.linear_insert(i);
    } else s.insertion(0, n);
}

}  // namespace sc
