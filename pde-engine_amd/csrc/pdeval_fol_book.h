// pdeval_fol_book.h -- the host bookkeeping of the foliation class registry (DESIGN.md §14
// "Registry"): class ids, keys, sizes, the capacity rule of the leader store and the merge of
// Stage A's first[] with Stage B's leaders into class ids, and the links between classes with
// the components they form (DESIGN.md §14 "Links and components").  Plain C++, no HIP: it
// compiles for the CPU as it is (tests/hostsim/sim_foliation_registry.cpp, guard_fol_registry.cpp,
// sim_foliation_link.cpp, guard_fol_links.cpp).
#pragma once
#include <algorithm>
#include <cstdint>
#include <iterator>
#include <utility>
#include <vector>

namespace pd {

// the leader store grows by doubling: the capacity that holds `need` leaders
inline int64_t fol_next_capacity(int64_t cap, int64_t need) {
    int64_t c = cap > 0 ? cap : 1;
    while (c < need) c *= 2;
    return c;
}

struct FolBook {
    std::vector<int64_t> keys, sizes;   // per class, in order of creation
    int64_t rows_seen = 0;              // rows assigned so far (the default key of the next row)
    // Links: unordered pairs of classes that share a member (a row that matches both leaders),
    // sorted, deduplicated, lo < hi.  parent: a union-find over class ids in which the smaller
    // root always becomes the root, so a component's root is its smallest class id.
    using Link = std::pair<int64_t, int64_t>;
    std::vector<Link> links;
    std::vector<int64_t> parent;

    int64_t n_classes() const { return (int64_t)keys.size(); }

    // Stage A's result is followed only if every entry is -1 or an index in [0, L)
    static bool first_ok(const int64_t* first, int64_t n, int64_t L) {
        for (int64_t r = 0; r < n; ++r)
            if (first[r] < -1 || first[r] >= L) return false;
        return true;
    }

    // the rows Stage B groups among themselves: unmatched by Stage A, enough finite points
    static void stage_b_rows(const int64_t* first, const int32_t* n_finite, int64_t n, int min_points,
                             std::vector<int64_t>& un) {
        un.clear();
        for (int64_t r = 0; r < n; ++r)
            if (first[r] < 0 && n_finite[r] >= min_points) un.push_back(r);
    }

    // The class ids of a batch, nothing changed yet.  first: Stage A (checked by first_ok);
    // leader_b[r]: the batch row that leads row r in Stage B, -1 for a row Stage B did not see.
    // Stage B's leaders are the rows with leader_b[r] == r; they get ids L, L + 1, ... in row
    // order (new_rows).  Returns false -- class_id and new_rows are then meaningless -- if
    // leader_b points outside the batch or at a row that is no leader.
    bool plan(const int64_t* first, const int64_t* leader_b, int64_t n, int64_t* class_id,
              std::vector<int64_t>& new_rows) const {
        const int64_t L = n_classes();
        new_rows.clear();
        for (int64_t r = 0; r < n; ++r) {
            const int64_t lb = leader_b[r];
            if (lb < -1 || lb >= n) return false;
            if (first[r] < 0 && lb == r) new_rows.push_back(r);
        }
        // (a leader precedes its members, so one pass in row order knows every leader's id)
        std::vector<int64_t> id_of((size_t)n, -1);
        for (size_t k = 0; k < new_rows.size(); ++k) id_of[(size_t)new_rows[k]] = L + (int64_t)k;
        for (int64_t r = 0; r < n; ++r) {
            if (first[r] >= 0) class_id[r] = first[r];
            else if (leader_b[r] < 0) class_id[r] = -1;
            else {
                const int64_t id = id_of[(size_t)leader_b[r]];
                if (id < 0) return false;
                class_id[r] = id;
            }
        }
        return true;
    }

    // the planned batch becomes part of the registry: new leaders appended with their keys (keys
    // == NULL: the running row number), sizes counted, rows_seen advanced
    void commit(const int64_t* class_id, int64_t n, const int64_t* row_keys, const std::vector<int64_t>& new_rows) {
        for (int64_t r : new_rows) {
            keys.push_back(row_keys ? row_keys[r] : rows_seen + r);
            sizes.push_back(0);
            parent.push_back((int64_t)parent.size());
        }
        for (int64_t r = 0; r < n; ++r)
            if (class_id[r] >= 0) ++sizes[(size_t)class_id[r]];
        rows_seen += n;
    }

    // saved leaders installed as they are; only into an empty registry
    bool load(const int64_t* leader_keys, const int64_t* leader_sizes, int64_t n) {
        if (n_classes() != 0 || rows_seen != 0 || n < 0) return false;
        for (int64_t k = 0; k < n; ++k)
            if (leader_sizes[k] < 0) return false;
        keys.assign(leader_keys, leader_keys + n);
        sizes.assign(leader_sizes, leader_sizes + n);
        parent.resize((size_t)n);
        for (int64_t k = 0; k < n; ++k) parent[(size_t)k] = k;
        for (int64_t k = 0; k < n; ++k) rows_seen += leader_sizes[k];
        return true;
    }

    // rows counted into existing classes without being assigned here (FoliationRegistry.merge)
    bool add_sizes(const int64_t* class_id, const int64_t* count, int64_t n) {
        for (int64_t k = 0; k < n; ++k)
            if (class_id[k] < 0 || class_id[k] >= n_classes() || count[k] < 0) return false;
        for (int64_t k = 0; k < n; ++k) {
            sizes[(size_t)class_id[k]] += count[k];
            rows_seen += count[k];
        }
        return true;
    }

    // ---- links and components
    // the component of class c: the smallest class id linked to it, directly or through others
    int64_t component(int64_t c) {
        while (parent[(size_t)c] != c) {
            parent[(size_t)c] = parent[(size_t)parent[(size_t)c]];   // (path halving: a parent is never larger)
            c = parent[(size_t)c];
        }
        return c;
    }
    int64_t n_components() const {
        int64_t n = 0;
        for (size_t c = 0; c < parent.size(); ++c) n += parent[c] == (int64_t)c;
        return n;
    }

    // The links of a call, nothing changed yet.  edges: n pairs of class ids (E = int32_t from the
    // link kernel's buffer, int64_t from a caller), in any order and with repeats; L: the classes
    // they may name (n_classes() after the batch they belong to).  Returns false -- an error of
    // the call, no entry is ever used as an index -- unless both ends of every pair lie in [0, L)
    // and differ.  merged: links plus the new pairs, sorted and deduplicated; fresh: the new
    // pairs alone.  Every allocation happens here, so a failure leaves the book as it was.
    template <class E>
    bool plan_links(const E* edges, int64_t n, int64_t L, std::vector<Link>& merged, std::vector<Link>& fresh) const {
        fresh.clear();
        if (n < 0) return false;
        for (int64_t k = 0; k < n; ++k) {
            const int64_t a = (int64_t)edges[2 * k], b = (int64_t)edges[2 * k + 1];
            if (a < 0 || a >= L || b < 0 || b >= L || a == b) return false;
            fresh.push_back(a < b ? Link{a, b} : Link{b, a});
        }
        std::sort(fresh.begin(), fresh.end());
        fresh.erase(std::unique(fresh.begin(), fresh.end()), fresh.end());
        std::vector<Link> kept;
        std::set_difference(fresh.begin(), fresh.end(), links.begin(), links.end(), std::back_inserter(kept));
        fresh.swap(kept);
        merged.clear();
        merged.reserve(links.size() + fresh.size());
        std::merge(links.begin(), links.end(), fresh.begin(), fresh.end(), std::back_inserter(merged));
        return true;
    }
    // the planned links become part of the book (after the commit of the batch that created the
    // classes they name): no allocation, components only ever merge
    void commit_links(std::vector<Link>& merged, const std::vector<Link>& fresh) {
        links.swap(merged);
        for (const Link& e : fresh) {
            const int64_t a = component(e.first), b = component(e.second);
            if (a != b) parent[(size_t)(a < b ? b : a)] = a < b ? a : b;
        }
    }
    // The links of another registry carried over by FoliationRegistry.merge: each of its n edges
    // mapped through id_map (its class id -> a class id here, n_map entries).  An edge whose ends
    // land in one class here links nothing and is dropped; that a merged leader joined an
    // existing class is no link by itself.  Returns false if an edge names a class outside
    // [0, n_map) or is a self edge there; the mapped ids are checked by plan_links.
    static bool map_links(const int64_t* edges, int64_t n, const int64_t* id_map, int64_t n_map,
                          std::vector<int64_t>& out) {
        out.clear();
        if (n < 0) return false;
        for (int64_t k = 0; k < n; ++k) {
            const int64_t a = edges[2 * k], b = edges[2 * k + 1];
            if (a < 0 || a >= n_map || b < 0 || b >= n_map || a == b) return false;
            if (id_map[a] == id_map[b]) continue;
            out.push_back(id_map[a]);
            out.push_back(id_map[b]);
        }
        return true;
    }
    // lim[] and cls[] of a link launch are followed only if cls[r] is -1 or in [0, L) and lim[r] in [0, L]
    static bool link_rows_ok(const int32_t* cls, const int32_t* lim, int64_t n, int64_t L) {
        for (int64_t r = 0; r < n; ++r)
            if (cls[r] < -1 || cls[r] >= L || lim[r] < 0 || lim[r] > L) return false;
        return true;
    }
    // lim[] of a committed batch (the arrival rule): the leaders that existed when row r was
    // assigned, L_before plus the new leaders positioned before it; 0 for an unclassified row.
    // new_rows: the batch rows that became leaders, ascending (plan).
    static void arrival_limits(const int64_t* class_id, int64_t n, int64_t L_before,
                               const std::vector<int64_t>& new_rows, std::vector<int32_t>& cls,
                               std::vector<int32_t>& lim) {
        cls.resize((size_t)n);
        lim.resize((size_t)n);
        size_t k = 0;
        for (int64_t r = 0; r < n; ++r) {
            while (k < new_rows.size() && new_rows[k] < r) ++k;
            cls[(size_t)r] = (int32_t)class_id[r];
            lim[(size_t)r] = class_id[r] < 0 ? 0 : (int32_t)(L_before + (int64_t)k);
        }
    }
};

}  // namespace pd
