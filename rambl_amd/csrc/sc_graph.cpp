// Host graph builder.  See sc_graph.hpp.  Each function cites the
// reference lines whose behaviour it reproduces
// (/root/reference/StrainCall/PartialOrderGraph.cpp unless another file is named).
#include "sc_graph.hpp"
#include "sc_phase_timer.hpp"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace sc {

static thread_local int tl_graph_threads = 1;
static thread_local long tl_graph_min_entries = 0;
void set_graph_threads(int n, long min_entries) {
    tl_graph_threads = n < 1 ? 1 : (n > 64 ? 64 : n);
    tl_graph_min_entries = min_entries;
}
int graph_threads(long entries) { return entries > tl_graph_min_entries ? tl_graph_threads : 1; }

// ---------------------------------------------------------------------------
void parse_cigar(const std::string& c, std::vector<CigarOp>& out) {   // cpp:13-59
    int v = 0;
    for (char ch : c) {
        switch (ch) {
            case 'M': case 'I': case 'D': case 'N': case 'S': case 'H': case 'P':
                out.push_back({ch, v}); v = 0; break;
            case '=': case 'X':
                out.push_back({'M', v}); v = 0; break;
            default:
                if (ch >= '0' && ch <= '9') v = v * 10 + (ch - '0');
        }
    }
}

int PoGraph::new_node(int st, const std::string& lab) {
    nodes.emplace_back();
    GNode& w = nodes.back();
    w.st = st; w.lab = lab;
    ++n_alive;
    return (int)nodes.size() - 1;
}
void PoGraph::add_edge(int u, int w) { nodes[u].out.push_back(w); nodes[w].in.push_back(u); }
void PoGraph::add_edge_gap(int u, const std::vector<int>& gap) {
    int a = u;
    for (int w : gap) { add_edge(a, w); a = w; }
}
void PoGraph::add_edge_gap_to(int u, int v, const std::vector<int>& gap) {
    add_edge_gap(u, gap);
    add_edge(gap.back(), v);
}
static inline void erase_first(std::vector<int>& v, int x) {
    auto it = std::find(v.begin(), v.end(), x);
    if (it != v.end()) v.erase(it);
}
void PoGraph::del_edge(int u, int v) { erase_first(nodes[u].out, v); erase_first(nodes[v].in, u); }
bool PoGraph::linking(int u, int v) const {
    const auto& o = nodes[u].out;
    return std::find(o.begin(), o.end(), v) != o.end();
}
// cpp:406-444; the O(N) erase + renumbering is replaced by a tombstone, ids are
// assigned once at the end (finalize_ids) -- the relative order is the same.
void PoGraph::delete_node(int w, bool bridging) {
    // note: in/out of w are not modified while we iterate them
    for (int p : nodes[w].in) {
        for (int c : nodes[w].out) {
            if (bridging && !linking(p, c)) add_edge(p, c);
            erase_first(nodes[c].in, w);
        }
        erase_first(nodes[p].out, w);
    }
    nodes[w].alive = false;
    --n_alive;
}

int PoGraph::reads_cover(int u, int v) const {
    const GNode &a = nodes[u], &b = nodes[v];
    int n = 0;
    if (u == 0) {
        for (const auto& e : b.pool) n += e.cn;
    } else if (b.lab == "$") {
        for (const auto& e : a.pool) n += e.cn;
    } else {
        // sum over pairs with equal rid of v's copy number; pools are rid-sorted in
        // practice, fall back to the quadratic form otherwise
        bool sorted = true;
        for (size_t i = 1; i < a.pool.size() && sorted; i++) sorted = a.pool[i - 1].rid <= a.pool[i].rid;
        for (size_t i = 1; i < b.pool.size() && sorted; i++) sorted = b.pool[i - 1].rid <= b.pool[i].rid;
        if (sorted) {
            size_t i = 0, j = 0;
            while (i < a.pool.size() && j < b.pool.size()) {
                if (a.pool[i].rid < b.pool[j].rid) i++;
                else if (a.pool[i].rid > b.pool[j].rid) j++;
                else {
                    int rid = a.pool[i].rid, mu = 0, sv = 0;
                    while (i < a.pool.size() && a.pool[i].rid == rid) { mu++; i++; }
                    while (j < b.pool.size() && b.pool[j].rid == rid) { sv += b.pool[j].cn; j++; }
                    n += mu * sv;
                }
            }
        } else {
            for (const auto& x : a.pool) for (const auto& y : b.pool) if (x.rid == y.rid) n += y.cn;
        }
    }
    return n;
}

// cpp:355-393
void PoGraph::find_insert_from(int u, std::vector<GapEx>& out) {
    std::vector<int> g, st;
    st.push_back(u);
    while (!st.empty()) {
        int v = st.back(); st.pop_back();
        if (v == u) {
            for (int o : nodes[v].out) if (nodes[o].st == ST_INS) st.push_back(o);
        } else if (nodes[v].st == ST_MAT || nodes[v].st == ST_MIS) {
            out.push_back({u, v, g});
            g.clear();
        } else {
            g.push_back(v);
            for (int o : nodes[v].out) st.push_back(o);
        }
    }
}

// cpp:780-829.  Sets of (rid, copies).
void PoGraph::find_common_read_pool(int a, int b, std::vector<std::pair<int, int>>& c) {
    auto build = [&](int x, const std::vector<int>& adj) {
        std::vector<std::pair<int, int>> s;
        s.reserve(nodes[x].pool.size());
        for (const auto& e : nodes[x].pool) s.emplace_back(e.rid, e.cn);
        std::sort(s.begin(), s.end());
        s.erase(std::unique(s.begin(), s.end()), s.end());
        std::vector<std::pair<int, int>> rm;
        for (int o : adj)
            if (nodes[o].st == ST_INS || nodes[o].st == ST_DEL)
                for (const auto& e : nodes[o].pool) rm.emplace_back(e.rid, e.cn);
        if (!rm.empty()) {
            std::sort(rm.begin(), rm.end());
            std::vector<std::pair<int, int>> kept;
            kept.reserve(s.size());
            std::set_difference(s.begin(), s.end(), rm.begin(), rm.end(), std::back_inserter(kept));
            s.swap(kept);
        }
        return s;
    };
    auto ar = build(a, nodes[a].out);
    auto br = build(b, nodes[b].in);
    c.clear();
    std::set_intersection(ar.begin(), ar.end(), br.begin(), br.end(), std::back_inserter(c));
}

void PoGraph::add_dash_chain(int a, int b, int l, const std::vector<std::pair<int, int>>& crp) {
    std::vector<int> gap;
    for (int t = 0; t < l; ++t) {
        int w = new_node(ST_INS, "-");
        auto& pool = nodes[w].pool;
        pool.reserve(crp.size());
        const int dash = intern("-");
        for (const auto& rc : crp) pool.push_back({rc.first, rc.second, dash});
        gap.push_back(w);
    }
    add_edge_gap_to(a, b, gap);
}
// cpp:831-923
void PoGraph::add_edge_level(int i, int l) {
    int u = i, v = i + 1;
    std::vector<std::pair<int, int>> crp;
    if (linking(u, v)) { find_common_read_pool(u, v, crp); add_dash_chain(u, v, l, crp); }
    { auto sv = nodes[v].sib;
      for (int s : sv) if (linking(u, s)) { find_common_read_pool(u, s, crp); add_dash_chain(u, s, l, crp); } }
    { auto su = nodes[u].sib;
      for (int s : su) if (linking(s, v)) { find_common_read_pool(s, v, crp); add_dash_chain(s, v, l, crp); } }
    { auto su = nodes[u].sib; auto sv = nodes[v].sib;
      for (int a : su) for (int b : sv)
          if (linking(a, b)) { find_common_read_pool(a, b, crp); add_dash_chain(a, b, l, crp); } }
}
// cpp:925-961
void PoGraph::delete_edge_level(int i) {
    int u = i, v = i + 1;
    if (linking(u, v)) del_edge(u, v);
    for (int s : nodes[v].sib) if (linking(u, s)) del_edge(u, s);
    for (int s : nodes[u].sib) if (linking(s, v)) del_edge(s, v);
    for (int a : nodes[u].sib) for (int b : nodes[v].sib) if (linking(a, b)) del_edge(a, b);
}

// cpp:446-550
void PoGraph::canonize_insert_at_level(int i) {
    std::vector<GapEx> found;
    find_insert_from(i, found);
    { auto sibs = nodes[i].sib; for (int s : sibs) find_insert_from(s, found); }
    if (found.empty()) return;
    int n = (int)found.size();
    std::vector<int> perm(n);
    for (int t = 0; t < n; t++) perm[t] = t;
    std_sort_perm(perm, [&](int a, int b) { return found[a].gap.size() > found[b].gap.size(); });
    std::vector<GapEx> inserts(n);
    for (int t = 0; t < n; t++) inserts[t] = std::move(found[perm[t]]);

    std::vector<std::string> seqs(n);
    int l = 0, k = 1000000000;
    for (int t = 0; t < n; t++) {
        for (int w : inserts[t].gap) seqs[t] += nodes[w].lab;
        l = std::max(l, (int)seqs[t].size());
        k = std::min(k, (int)seqs[t].size());
    }
    if (n == 1 || l - k == 0) {
        add_edge_level(i, l);
        delete_edge_level(i);
        return;
    }
    std::vector<std::string> rows;
    int ncol = msa_(seqs, rows);
    ++msa_calls;
    for (int t = 0; t < n; ++t) {
        if (rows[t] != seqs[t]) {
            int rid = 0, rcn = 0;
            for (int w : inserts[t].gap) {
                rid = nodes[w].pool[0].rid;
                rcn = nodes[w].pool[0].cn;
                delete_node(w, true);
            }
            std::vector<int> ng;
            for (char ch : rows[t]) {
                std::string lab(1, ch);
                int w = new_node(ST_INS, lab);
                nodes[w].pool.push_back({rid, rcn, intern(lab)});
                ng.push_back(w);
            }
            add_edge_gap_to(inserts[t].u, inserts[t].v, ng);
        }
    }
    add_edge_level(i, ncol);
    delete_edge_level(i);
}

// cpp:571-622
// The level at which the walk below first takes w off its list is w's distance from the root over the edges the walk
// follows (out-edges to nodes that are no deletions, and the siblings of those nodes).  While canonize_delete runs,
// these edges do not change -- it only adds deletion nodes and edges into them -- so one breadth-first pass serves every
// query of the phase (723 walks over 400 000 nodes on the unthinned configs[3] region otherwise).
void PoGraph::level_cache_build() {
    level_cache_.assign(nodes.size(), -1);
    std::vector<int> cur{0}, nxt;
    level_cache_[0] = 0;
    int level = 0;
    while (!cur.empty()) {
        level += 1;
        nxt.clear();
        for (int u : cur)
            for (int o : nodes[u].out) {
                if (nodes[o].st == ST_DEL) continue;
                if (level_cache_[o] < 0) { level_cache_[o] = level; nxt.push_back(o); }
                for (int s : nodes[o].sib) if (level_cache_[s] < 0) { level_cache_[s] = level; nxt.push_back(s); }
            }
        cur.swap(nxt);
    }
}
int PoGraph::node_level_exclude_delete(int w) {
    if (level_cache_on_ && w < (int)level_cache_.size() && level_cache_[w] >= 0) return level_cache_[w];
    std::vector<int> level_node, sub;
    int level = 0;
    int stamp = ++stamp_;
    level_node.push_back(0);
    while (!level_node.empty()) {
        int u = level_node.back(); level_node.pop_back();
        if (u == w) break;
        for (int o : nodes[u].out) {
            if (nodes[o].st == ST_DEL) continue;
            sub.push_back(o);
            for (int s : nodes[o].sib) sub.push_back(s);
        }
        if (level_node.empty()) {
            while (!sub.empty()) {
                int v = sub.back(); sub.pop_back();
                if (nodes[v].stamp_a == stamp) continue;
                level_node.push_back(v);
                nodes[v].stamp_a = stamp;
            }
            level += 1;
            stamp = ++stamp_;
        }
    }
    return level;
}
// cpp:624-672
void PoGraph::find_delete_from(int w, std::vector<GapEx>& out) {
    std::vector<int> gap, st, cnt;
    st.push_back(w); cnt.push_back(0);
    while (!st.empty()) {
        int u = st.back(); st.pop_back();
        int c = cnt.back(); cnt.pop_back();
        if (u == w) {
            for (int o : nodes[u].out) if (nodes[o].st == ST_DEL) { st.push_back(o); cnt.push_back(0); }
        } else if (nodes[u].st == ST_DEL) {
            if (c == 0) {
                st.push_back(u); cnt.push_back(1);
                gap.push_back(u);
                for (int o : nodes[u].out) { st.push_back(o); cnt.push_back(0); }
            } else gap.pop_back();
        } else {
            out.push_back({w, u, gap});
        }
    }
}
// cpp:684-740
void PoGraph::canonize_delete_at_level(int i) {
    std::vector<GapEx> deletes;
    find_delete_from(i, deletes);
    { auto sibs = nodes[i].sib; for (int s : sibs) find_delete_from(s, deletes); }
    if (deletes.empty()) return;
    std::vector<std::pair<int, int>> nl;   // node -> level cache, local to this call
    auto level_of = [&](int x) {
        for (auto& p : nl) if (p.first == x) return p.second;
        int lv = node_level_exclude_delete(x);
        nl.emplace_back(x, lv);
        return lv;
    };
    for (auto& d : deletes) {
        int ul = level_of(d.u), vl = level_of(d.v);
        int dl = vl - ul - 1, dd = (int)d.gap.size();
        if (dl - dd > 0) {
            int v0 = d.gap[0];
            int rid = nodes[v0].pool[0].rid, rcn = nodes[v0].pool[0].cn;
            std::vector<int> ng;
            for (int t = dl - dd; t > 0; --t) {
                int w = new_node(ST_DEL, "=");
                nodes[w].pool.push_back({rid, rcn, intern("=")});
                ng.push_back(w);
            }
            add_edge_gap_to(d.u, v0, ng);
            del_edge(d.u, v0);
        }
    }
}

// cpp:963-1005
int PoGraph::intern(const std::string& lab) {
    auto it = lab_id_.find(lab);
    if (it != lab_id_.end()) return it->second;
    const int id = (int)labtab.size();
    labtab.push_back(lab);
    lab_id_.emplace(lab, id);
    return id;
}
int PoGraph::concat(int a, int b) {
    const unsigned long long key = ((unsigned long long)(unsigned)a << 32) | (unsigned)b;
    auto it = lab_cat_.find(key);
    if (it != lab_cat_.end()) return it->second;
    const int id = intern(labtab[(size_t)a] + labtab[(size_t)b]);
    lab_cat_.emplace(key, id);
    return id;
}
void PoGraph::merge_read_pool(int u, int v) {
    auto cmp = [this](const PoolEnt& a, const PoolEnt& b) {
        if (a.rid != b.rid) return a.rid < b.rid;
        if (a.lab != b.lab) return labtab[(size_t)a.lab] < labtab[(size_t)b.lab];
        return a.cn < b.cn;
    };
    auto& pu = nodes[u].pool;
    auto& pv = nodes[v].pool;
    if (!std::is_sorted(pu.begin(), pu.end(), cmp)) std::sort(pu.begin(), pu.end(), cmp);
    if (!std::is_sorted(pv.begin(), pv.end(), cmp)) std::sort(pv.begin(), pv.end(), cmp);
    std::vector<PoolEnt> res;
    res.reserve(pu.size() + pv.size());
    size_t i = 0, j = 0;
    while (i < pu.size() && j < pv.size()) {
        if (pu[i].rid == pv[j].rid) {
            res.push_back({pu[i].rid, pu[i].cn, concat(pu[i].lab, pv[j].lab)});
            i++; j++;
        } else if (pu[i].rid < pv[j].rid) res.push_back(pu[i++]);
        else res.push_back(pv[j++]);
    }
    res.insert(res.end(), pu.begin() + (long)i, pu.end());
    res.insert(res.end(), pv.begin() + (long)j, pv.end());
    pu.swap(res);
}
// cpp:1007-1038
void PoGraph::merge_node(int u, int v) {
    { auto vin = nodes[v].in;
      for (int p : vin) if (!linking(p, u) && p != u) add_edge(p, u); }
    { auto vout = nodes[v].out;
      for (int c : vout) if (!linking(u, c) && u != c) add_edge(u, c); }
    if (linking(u, v) && nodes[u].st == ST_MAT && nodes[v].st == ST_MAT) nodes[u].lab += nodes[v].lab;
    merge_read_pool(u, v);
    delete_node(v, false);
    std::vector<PoolEnt>().swap(nodes[v].pool);
}
// cpp:1040-1094 / 1097-1159
void PoGraph::directional_merge(bool backward) {
    std::vector<int> q;
    size_t qh = 0;
    int st_merged = ++stamp_, st_visit = ++stamp_;
    if (!backward) q.push_back(0);
    else for (int i = 0; i < (int)nodes.size(); i++) if (nodes[i].alive && nodes[i].lab == "$") q.push_back(i);
    std::vector<std::pair<int, int>> to_merge;
    while (qh < q.size()) {
        int w = q[qh++];
        if (nodes[w].stamp_a == st_merged) continue;
        {
            const auto& adj = backward ? nodes[w].in : nodes[w].out;
            for (size_t a = 0; a < adj.size(); a++) {
                int u = adj[a];
                for (size_t b = a + 1; b < adj.size(); b++) {
                    int v = adj[b];
                    if (u == v) continue;
                    if (nodes[u].st == nodes[v].st && nodes[u].lab == nodes[v].lab)
                        if (nodes[u].stamp_a != st_merged && nodes[v].stamp_a != st_merged) {
                            to_merge.emplace_back(u, v);
                            nodes[v].stamp_a = st_merged;
                        }
                }
            }
        }
        for (auto& m : to_merge) merge_node(m.first, m.second);
        to_merge.clear();
        const auto& adj = backward ? nodes[w].in : nodes[w].out;
        for (int c : adj)
            if (nodes[c].stamp_b != st_visit) { q.push_back(c); nodes[c].stamp_b = st_visit; }
    }
}
// cpp:1171-1216
void PoGraph::path_collapse() {
    int level_size = 0;
    std::vector<int> lq, sq;
    size_t lh = 0;
    int stamp = ++stamp_;
    lq.push_back(0);
    while (lh < lq.size()) {
        int u = lq[lh++];
        if (level_size == 1 && nodes[u].out.size() == 1) {
            int v = nodes[u].out[0];
            while (nodes[v].out.size() == 1) {
                merge_node(u, v);
                v = nodes[u].out[0];
            }
        }
        for (int v : nodes[u].out)
            if (nodes[v].stamp_c != stamp) { sq.push_back(v); nodes[v].stamp_c = stamp; }
        if (lh == lq.size()) {
            lq.swap(sq); sq.clear(); lh = 0;
            level_size = (int)lq.size();
            stamp = ++stamp_;
        }
    }
}
// cpp:769-776 + LevelOrderIterator.cpp:3-56
void PoGraph::node_level() {
    std::vector<int> level_node, sub;
    int n = 0, level = 0, stamp = ++stamp_;
    int cur = 0, cur_level = 0;
    for (int o : nodes[0].out) level_node.push_back(o);
    nodes[0].stamp_a = stamp;
    while (n != n_alive) {
        nodes[cur].level = cur_level;
        if (sub.empty()) { level += 1; stamp = ++stamp_; }
        if (!level_node.empty()) {
            int w = level_node.back(); level_node.pop_back();
            cur = w; cur_level = level;
            n += 1;
            for (int o : nodes[w].out) sub.push_back(o);
            if (level_node.empty()) {
                while (!sub.empty()) {
                    int x = sub.back(); sub.pop_back();
                    if (nodes[x].stamp_a == stamp) continue;
                    level_node.push_back(x);
                    nodes[x].stamp_a = stamp;
                }
            }
        } else n += 1;
    }
}
void PoGraph::finalize_ids() {
    order_.clear();
    for (int i = 0; i < (int)nodes.size(); i++)
        if (nodes[i].alive) { nodes[i].id = (int)order_.size(); order_.push_back(i); }
}

// ---------------------------------------------------------------------------
// cpp:94-255, the read loop.  The per-base work (class of every M-aligned base,
// pools, first read of every class / transition) comes from the device tables;
// thread_reads replays node creations and add_edge calls in the order the
// reference makes them -- by read, then by position inside the read -- and walks
// only the reads that contain insertions or deletions (their private chains).
namespace {
const int INF = 0x7fffffff;
enum { EV_SIB = 0, EV_CHAIN = 1, EV_EDGE = 2 };
enum { REF_CLASS = 0, REF_NODE = 1, REF_CHAIN = 2 };
struct NodeRef { int type, a, b; };                     // CLASS: (i, c); NODE: node index; CHAIN: (chain id, position)
struct Event {
    int rid, op, t, kind;                               // the order of the replay: read, operation, offset, kind
    int i, c;                                           // EV_SIB
    int chain;                                          // EV_CHAIN
    NodeRef u, v; bool force, check_ne;                 // EV_EDGE
};
struct Chain { int st; std::string labels; int rid; std::vector<int> nodes; };
const int OP_LAST = 1 << 29;                            // after every operation of the read
NodeRef class_ref(int i, int c) { return NodeRef{REF_CLASS, i, c}; }
NodeRef node_ref(int w) { return NodeRef{REF_NODE, w, 0}; }
NodeRef chain_ref(int cid, int at) { return NodeRef{REF_CHAIN, cid, at}; }
Event sib_event(int rid, int op, int t, int i, int c) { return Event{rid, op, t, EV_SIB, i, c, 0, {}, {}, false, false}; }
Event chain_event(int rid, int op, int chain) { return Event{rid, op, 0, EV_CHAIN, 0, 0, chain, {}, {}, false, false}; }
Event edge_event(int rid, int op, int t, NodeRef u, NodeRef v, bool force, bool check_ne) {
    return Event{rid, op, t, EV_EDGE, 0, 0, 0, u, v, force, check_ne};
}
}  // namespace

struct PoGraph::Threading {
    PoGraph& g;
    const std::string& G;
    const std::vector<AlignedRead>& R;
    const int glen, n;
    std::vector<std::vector<CigarOp>> cig;
    std::vector<char> complex_read;                     // the read carries I or D
    ThreadTables T;
    std::vector<Event> ev;
    size_t n_class_events = 0;
    std::vector<Chain> chains;
    std::vector<int> class_node;                        // [glen*8] node of a class, -1 before its sibling exists

    Threading(PoGraph& g, const std::string& G, const std::vector<AlignedRead>& R)
        : g(g), G(G), R(R), glen((int)G.size()), n((int)R.size()), cig((size_t)n), complex_read((size_t)n, 0) {
        for (int r = 0; r < n; r++) {
            parse_cigar(R[r].cigar, cig[r]);
            for (const CigarOp& c : cig[r]) {
                if (c.op == 'I' || c.op == 'D') complex_read[r] = 1;
                else if (c.op != 'M') throw std::runtime_error("CIGAR operation other than M/I/D/=/X in a cropped read");
            }
        }
    }
    int ref_code(int i) const { return (int)T.lut[(unsigned char)G[i]]; }
    // (op index, offset) of reference position i inside read r, for ordering
    void locate(int r, int i, int& op, int& t) const {
        if (!complex_read[r]) { op = 0; t = i - R[r].pos; return; }
        int ri = R[r].pos;
        for (int k = 0; k < (int)cig[r].size(); k++) {
            const CigarOp& c = cig[r][k];
            if (c.op == 'M') { if (i < ri + c.len) { op = k; t = i - ri; return; } ri += c.len; }
            else if (c.op == 'D') ri += c.len;
        }
        op = (int)cig[r].size(); t = 0;
    }
    void class_events();
    void chain_events(int r);
    void sort_events();
    void replay();
    void fill_pools();
};

// Events of the class tables: the sibling of every "mis" class and the first read over every edge between classes.
void PoGraph::Threading::class_events() {
    for (int i = 0; i < glen; i++) {
        const int gc = ref_code(i);
        for (int c = 0; c < 8; c++) {
            const int cls = i * 8 + c;
            if (T.count[cls] == 0) continue;
            int op, t;
            if (c != gc) {                               // first read of a "mis" class creates the sibling (:151-163)
                locate(T.minrid[cls], i, op, t);
                ev.push_back(sib_event(T.minrid[cls], op, t, i, c));
            }
            if (T.smin[cls] != INF && c != gc) {         // read starts here: edge from the backbone node before it
                const int r = T.smin[cls];
                ev.push_back(edge_event(r, 0, 0, node_ref(R[r].pos), class_ref(i, c), false, false));
            }
            if (T.emin[cls] != INF && c != gc)           // read ends here: edge to the next backbone node (:252-253)
                ev.push_back(edge_event(T.emin[cls], OP_LAST, 0, class_ref(i, c), node_ref(i + 2), false, true));
            if (i == 0) continue;
            const int gp = ref_code(i - 1);
            for (int cp = 0; cp < 8; cp++) {
                const int r = T.tmin[i * 64 + cp * 8 + c];
                if (r == INF || (cp == gp && c == gc)) continue;    // backbone -> backbone is linked from the start
                locate(r, i, op, t);
                ev.push_back(edge_event(r, op, t, class_ref(i - 1, cp), class_ref(i, c), false, false));
            }
        }
    }
    n_class_events = ev.size();
}

// Events of one read with insertions / deletions: its private chains and the edges around them.
void PoGraph::Threading::chain_events(int r) {
    const AlignedRead& rd = R[r];
    const int rlen = (int)rd.seq.size();
    int i = rd.pos, j = 0;
    NodeRef u = node_ref(rd.pos);                        // nodes[pos]: the backbone node before the first base
    const int nops = (int)cig[r].size();
    for (int k = 0; k < nops; k++) {
        const CigarOp& c = cig[r][k];
        if (c.op == 'M') {
            if (i + c.len > glen || j + c.len > rlen) throw std::runtime_error("read runs past the window");
            const int cfirst = T.lut[(unsigned char)rd.seq[j]];
            if (k > 0 && cig[r][k - 1].op != 'M')        // first base after a chain: edge from its tail (:141-174)
                ev.push_back(edge_event(r, k, 0, u, class_ref(i, cfirst), false, false));
            i += c.len; j += c.len;
            u = class_ref(i - 1, T.lut[(unsigned char)rd.seq[j - 1]]);
            continue;
        }
        Chain ch; ch.rid = r;
        if (c.op == 'I') {
            if (j + c.len > rlen) throw std::runtime_error("insertion runs past the read");
            ch.st = ST_INS; ch.labels = rd.seq.substr(j, c.len); j += c.len;
        } else {
            ch.st = ST_DEL; ch.labels = std::string((size_t)c.len, '='); i += c.len;
            if (i > glen) throw std::runtime_error("deletion runs past the window");
        }
        const int cid = (int)chains.size();
        chains.push_back(ch);
        ev.push_back(chain_event(r, k, cid));
        ev.push_back(edge_event(r, k, 0, u, chain_ref(cid, 0), true, false));               // add_edge(u, gap) (:190, :217)
        u = chain_ref(cid, c.len - 1);
        if (c.op == 'D' && i == glen) {                                                     // deletion up to "$" (:209-215)
            ev.push_back(edge_event(r, k, 1, u, node_ref(glen + 1), true, false));
            u = node_ref(glen + 1);
        }
    }
    if (nops > 0 && cig[r][nops - 1].op != 'M') {        // final `if (!linking(u,v) and u!=v) add_edge(u,v)` (:252-253)
        if (i + 1 >= (int)g.nodes.size()) throw std::runtime_error("read runs past the window");
        ev.push_back(edge_event(r, OP_LAST, 0, u, node_ref(i + 1), false, true));
    }
}

// The events of the reads were made in read and operation order: sort the few class events, merge (the same order as one
// stable sort of everything).
void PoGraph::Threading::sort_events() {
    auto ev_less = [](const Event& a, const Event& b) {
        if (a.rid != b.rid) return a.rid < b.rid;
        if (a.op != b.op) return a.op < b.op;
        if (a.t != b.t) return a.t < b.t;
        return a.kind < b.kind;
    };
    if (std::is_sorted(ev.begin() + (long)n_class_events, ev.end(), ev_less)) {
        std::stable_sort(ev.begin(), ev.begin() + (long)n_class_events, ev_less);
        std::inplace_merge(ev.begin(), ev.begin() + (long)n_class_events, ev.end(), ev_less);
    } else {
        std::stable_sort(ev.begin(), ev.end(), ev_less);
    }
}

// Node creations and add_edge calls in the order the reference makes them.
void PoGraph::Threading::replay() {
    class_node.assign((size_t)glen * 8, -1);
    for (int i = 0; i < glen; i++) if (ref_code(i) < 8) class_node[(size_t)i * 8 + ref_code(i)] = i + 1;   // a gene base no read carries has no class
    auto resolve = [&](const NodeRef& x) -> int {
        if (x.type == REF_NODE) return x.a;
        if (x.type == REF_CLASS) return class_node[(size_t)x.a * 8 + x.b];
        return chains[x.a].nodes[x.b];
    };
    for (const Event& e : ev) {
        if (e.kind == EV_SIB) {
            const int w = g.new_node(ST_MIS, std::string(1, T.sym[e.c]));
            g.nodes[e.i + 1].sib.push_back(w);
            class_node[(size_t)e.i * 8 + e.c] = w;
        } else if (e.kind == EV_CHAIN) {
            Chain& ch = chains[e.chain];
            int prev = -1;
            for (char lab : ch.labels) {
                const int w = g.new_node(ch.st, std::string(1, lab));
                g.nodes[w].pool.push_back({ch.rid, R[ch.rid].cn, g.intern(std::string(1, lab))});
                if (prev >= 0) g.add_edge(prev, w);
                ch.nodes.push_back(w);
                prev = w;
            }
        } else {
            const int a = resolve(e.u), b = resolve(e.v);
            if (a < 0 || b < 0) throw std::runtime_error("edge event before its node");
            if (e.force || (!g.linking(a, b) && !(e.check_ne && a == b))) g.add_edge(a, b);
        }
    }
}

// Pools of the backbone / sibling nodes, in read order (a million entries: copy numbers from a compact array, written by
// index).  A class has a node of its own: the pools fill independently of each other (on a deep region this is 88 M entries).
void PoGraph::Threading::fill_pools() {
    std::vector<int> copies((size_t)n);
    for (int r = 0; r < n; r++) copies[(size_t)r] = R[r].cn;
    int sym_lab[8];
    for (int c = 0; c < 8; c++) sym_lab[c] = c < (int)T.sym.size() ? g.intern(std::string(1, T.sym[c])) : -1;
    for (int cls = 0; cls < glen * 8; cls++)
        if (T.count[cls] != 0 && class_node[cls] < 0) throw std::runtime_error("class without a node");
    parallel_items(glen * 8, graph_threads((long)T.pool.size()), [&](int cls) {
        if (T.count[cls] == 0) return;
        auto& pool = g.nodes[class_node[cls]].pool;
        const int lab = sym_lab[cls & 7];
        const size_t at = pool.size(), cnt = (size_t)(T.off[cls + 1] - T.off[cls]);
        pool.resize(at + cnt);
        PoolEnt* dst = pool.data() + at;
        const int* src = T.pool.data() + T.off[cls];
        for (size_t x = 0; x < cnt; x++) dst[x] = PoolEnt{src[x], copies[(size_t)src[x]], lab};
    });
}

void PoGraph::thread_reads(const std::string& G, const std::vector<AlignedRead>& R, const ThreadFn& thread) {
    PhaseTimer tp("    thread_reads ", 14);
    Threading t(*this, G, R);
    tp.phase("cigars");
    thread(G, R, t.cig, t.T);
    tp.phase("thread stage");
    if ((int)t.T.sym.size() > 8) throw std::runtime_error("more than 8 distinct symbols in the reads");
    t.class_events();
    for (int r = 0; r < t.n; r++) if (t.complex_read[r]) t.chain_events(r);
    tp.phase("events");
    t.sort_events();
    tp.phase("event sort");
    t.replay();
    tp.phase("replay");
    t.fill_pools();
    tp.phase("pools");
}

// cpp:67-265
PoGraph::PoGraph(const std::string& G, const std::vector<AlignedRead>& R, const MsaFn& msa, const ThreadFn& thread) : msa_(msa) {
    const int glen = (int)G.size();
    nodes.reserve((size_t)glen + 2 + R.size() / 2);
    int u = new_node(ST_MAT, "^");
    for (int i = 0; i < glen; i++) {
        int w = new_node(ST_MAT, std::string(1, G[i]));
        add_edge(u, w);
        u = w;
    }
    int E = new_node(ST_MAT, "$");
    add_edge(u, E);
    PhaseTimer tp("  graph phase ", 18);
    thread_reads(G, R, thread);
    tp.phase("thread_reads");
    // canonize_graph, cpp:754-767
    for (int i = 0; i < (int)nodes.size(); ++i) {            // canonize_insert :553-564
        if (nodes[i].lab == "$") break;
        canonize_insert_at_level(i);
    }
    tp.phase("canonize_insert");
    level_cache_build();
    level_cache_on_ = true;
    for (int i = 0; i < (int)nodes.size(); ++i) {            // canonize_delete :742-752
        if (nodes[i].lab == "$") break;
        canonize_delete_at_level(i);
    }
    level_cache_on_ = false;
    std::vector<int>().swap(level_cache_);
    tp.phase("canonize_delete");
    directional_merge(false);
    tp.phase("forward_merge");
    directional_merge(true);
    tp.phase("backward_merge");
    path_collapse();
    tp.phase("path_collapse");
    finalize_ids();
    node_level();
    tp.phase("ids + levels");
}

std::string PoGraph::dump() const {
    std::string s;
    char buf[64];
    for (int i : order_) {
        const GNode& x = nodes[i];
        int rc = 0;
        for (const auto& e : x.pool) rc += e.cn;
        snprintf(buf, sizeof buf, "#\t%d\t%d\t", x.id, x.level);
        s += buf; s += x.lab;
        snprintf(buf, sizeof buf, "\t%d\n", rc);
        s += buf;
    }
    for (int i : order_) {
        const GNode& x = nodes[i];
        for (int o : x.out) {
            snprintf(buf, sizeof buf, "%d\t%d\t%d\n", x.id, nodes[o].id, reads_cover(i, o));
            s += buf;
        }
    }
    return s;
}

}  // namespace sc
