// A lane pass of the conv net as a scope.  Between the first use_lane(k) of a pass and its lanes_join() the net's workspace pointers
// and the HANDLE's stream are lane k's (net_conv.hip: use_lane), so every way out of the pass has to go through lanes_join(), which
// makes lane 0 -- the handle's own stream -- current again; env steps of the handle would otherwise be enqueued on a lane stream.
// The guard owes that join from its construction on: an early `return rc` pays it in the destructor (behind the return expression;
// its result is ignored: the caller hears the error that ended the pass), the success path pays it with finish() and gets its code.
// Plain C++ (no HIP), so that a host program can hold it to a counting net (tests/test_lane_scope.py).  Net: any type for which
// lanes_fork(Net *) and lanes_join(Net *) are declared before this header is included.
#pragma once

namespace grl {

template <class Net>
struct LanePass {
    Net *const net;
    bool owed = true;
    explicit LanePass(Net *n) : net(n) {}      // a pass that makes its lanes current itself (use_lane in a loop) constructs and never begins
    LanePass(const LanePass &) = delete;
    ~LanePass() { if (owed) (void)lanes_join(net); }
    int begin() { return lanes_fork(net); }      // the lanes see what is enqueued on lane 0 so far; a failure leaves the join owed
    int finish() { owed = false; return lanes_join(net); }      // the one join of the success path
    void dismiss() { owed = false; }      // no lane was ever made current: nothing to join (no caller yet; tests/test_lane_scope.py holds it)
};

}  // namespace grl
