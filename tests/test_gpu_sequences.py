"""Random call sequences over every stepping path of one engine, on the device, against the one model of tests/sequence_ref.py.

Every committed sequence (sequence_ref.sequences(): 12 to 16 calls on an engine of 1 to 4200 lanes, drawn so that every ordered pair
of stepping paths, every event before every kind of launch, every flag set, both lanes-per-work-item shapes and the engines whose
arrays live in mapped host memory all occur) is replayed call by call on the library and on the model (tests/sequence_replay.py).
After EVERY call the state, the observation, reward / done / truncated, the final observations, the tick, the statistics, the
per-policy records and every row of a recording launch equal the model bit for bit (a NaN equal to any NaN; Pendulum's sum of returns
to rtol 1e-5), the padding lanes of the record buffers still hold their sentinel, and a refused call has changed nothing.  At the end
of every sequence the zero-copy views (state, obs, reward, done, truncated, final observations, the statistics' four doubles) are
read on the engine's stream and equal the host copies byte for byte.  Nothing writes into the views; no environment variable, no
subprocess, no invalid action.

tests/test_sequence_ref.py shows without a GPU that the model is the existing references where a sequence stays inside one
family, that the list covers what it claims, and that six planted hand-over faults would each fail a sequence here.
A failing sequence is data: copy it into FIXED below, shorten it there (drop ops, halve steps), and keep the shortest."""
import pytest
import sequence_ref as sq
import sequence_replay

pytestmark = pytest.mark.gpu

SEQUENCES = sq.sequences()

# Named, fixed cases: the shortest form of every sequence that ever failed here, (name, Config, ops).  None so far.
FIXED = ()


@pytest.mark.parametrize("k", range(len(SEQUENCES)), ids=[sq.sequence_id(k, c) for k, (c, _) in enumerate(SEQUENCES)])
def test_sequence_equals_the_model_after_every_call(gymrs, k):
    c, ops = SEQUENCES[k]
    sequence_replay.replay(gymrs, c, ops)


if FIXED:
    @pytest.mark.parametrize("name,c,ops", FIXED, ids=[f[0] for f in FIXED])
    def test_fixed_sequence(gymrs, name, c, ops):
        sequence_replay.replay(gymrs, c, ops)
