"""MI355X-native hot path of LLMRec Stage 2: the C-ABI HIP library (csrc/, lib/) and its Python host side."""
import os

# ROCm's hipGraphLaunch gives a multi-branch graph's internal streams to its branches and skips every internal stream that shares a HARDWARE
# queue with the launch stream - without a bounds check ("HIP graph launch and hardware queues"). With the runtime's
# default pool of hardware queues two of an executable's internal streams can land on the launch stream's queue, and the launch then walks
# off the stream vector (a host-side segfault that depended on every stream the process had created before). A graph with ONE branch uses
# no internal stream, so every graph this package captures is single-branch: FusedStep captures on one stream (LLMREC_STREAMS defaults to
# 0), and a capture of a multi-branch step (LLMREC_STREAMS=1 with graph replay) is REFUSED unless LLMREC_UNSAFE_GRAPH=1 overrides.
# Eager launches (LLMREC_GRAPH=0) may use several streams: the fault is the graph launch's own.


def multi_branch_graphs_allowed() -> bool:
    """True only with LLMREC_UNSAFE_GRAPH=1: the caller takes responsibility for hipGraphLaunch of a multi-branch graph (see above)."""
    return os.environ.get("LLMREC_UNSAFE_GRAPH", "0") == "1"


def require_graph_replay(what: str, multi_branch: bool):
    """Raise if a stream capture would record a multi-branch graph and LLMREC_UNSAFE_GRAPH=1 does not allow it (every capture calls this)."""
    if multi_branch and not multi_branch_graphs_allowed():
        raise RuntimeError("%s: capture of a multi-branch HIP graph refused - hipGraphLaunch of a multi-branch graph can fault on the host "
                           "(DESIGN.md section 4); set LLMREC_STREAMS=0 (the default) for a single-branch graph, or LLMREC_GRAPH=0 for "
                           "eager launches on several streams" % what)
