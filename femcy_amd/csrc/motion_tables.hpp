// The tables of femcy_explicit_set_motion, built once on the host for both backends of the C ABI: the compact list of moved
// DOFs (index, value, curve), the per-DOF index into it (-1: not moved) that the node pass reads, and the distinct curves in
// the order of their first use.  A DOF named by two sets keeps its place in the list and takes the later set's value and
// curve, so every DOF stands in the list once and no two lanes write the same entry.  Host-only, no HIP types.
#pragma once
#include <stdint.h>
#include <vector>
#include "element_math.hpp"

namespace femcy {

struct MotionTables {
    std::vector<int32_t> slot;      // [n] position in dof / val / curve, -1: not moved
    std::vector<int32_t> dof, curve;
    std::vector<double> val;
    std::vector<Amplitude> amp;     // the distinct curves, at most FEMCY_MOTION_MAX_CURVES (check_explicit_set_motion)
};

// sets[k]: the DOFs of the k-th set; amps: the context's amplitudes, indexed by amplitude_ids[k]
inline MotionTables motion_tables(int64_t n, const std::vector<std::vector<int32_t>>& sets, const double* values,
                                  const int32_t* amplitude_ids, const std::vector<Amplitude>& amps) {
    MotionTables m;
    m.slot.assign((size_t)n, -1);
    std::vector<int32_t> ids;
    for (size_t k = 0; k < sets.size(); ++k) {
        size_t j = 0;
        while (j < ids.size() && ids[j] != amplitude_ids[k]) ++j;
        if (j == ids.size()) {
            ids.push_back(amplitude_ids[k]);
            m.amp.push_back(amps[(size_t)amplitude_ids[k]]);
        }
        for (int32_t d : sets[k]) {
            int32_t& s = m.slot[(size_t)d];
            if (s < 0) {
                s = (int32_t)m.dof.size();
                m.dof.push_back(d);
                m.val.push_back(values[k]);
                m.curve.push_back((int32_t)j);
            } else {
                m.val[(size_t)s] = values[k];
                m.curve[(size_t)s] = (int32_t)j;
            }
        }
    }
    return m;
}

}  // namespace femcy
