"""NumPy restatement of the inference end-detection rule (include/taco_hip.h, TacoStopRule) for the tests."""
import numpy as np


def stop_lengths(alignments, text_length, end_offset, hold, min_steps):
    """alignments (B, Td, Tt), text_length (B) -> len_b (B) int32.
    target = max(0, L - 1 - end_offset) with L clamped to 1..Tt; a_t = np.argmax(alignments[b, t, :Tt]) (lowest index on ties);
    run_t = run_{t-1} + 1 if a_t >= target else 0; t* = first t with run_t >= hold and t + 1 >= min_steps;
    len_b = min(Td, 4 ceil((t* + 1) / 4)), Td without such a t."""
    al = np.asarray(alignments)
    B, Td, Tt = al.shape
    out = np.full(B, Td, dtype=np.int32)
    for b in range(B):
        L = min(max(int(text_length[b]), 1), Tt)
        target = max(0, L - 1 - end_offset)
        run = 0
        for t in range(Td):
            run = run + 1 if int(np.argmax(al[b, t, :Tt])) >= target else 0
            if run >= hold and t + 1 >= min_steps:
                out[b] = min(Td, 4 * ((t + 1 + 3) // 4))
                break
    return out
