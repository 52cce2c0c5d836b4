// pdeval_fol_book.h -- the host bookkeeping of the foliation class registry (DESIGN.md §14
// "Registry"): class ids, keys, sizes, the capacity rule of the leader store and the merge of
// Stage A's first[] with Stage B's leaders into class ids.  Plain C++, no HIP: it compiles for
// the CPU as it is (tests/hostsim/sim_foliation_registry.cpp, guard_fol_registry.cpp).
#pragma once
#include <cstdint>
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
};

}  // namespace pd
