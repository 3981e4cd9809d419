"""transfer_leadership in a closed loop through ra_amd.shell.RaShell: the call to the leader, its reply to the caller,
the {send_msg, Target, election_timeout, cast} the shell routes to the target, the target's election, and the old
leader's await condition released by the new leader's higher-term append_entries_rpc -- or, when the target is cut
off, ended by the condition's timeout (back to leader).  Then a drain: every leader moved off one member slot."""
import pytest

from ra_amd import abi
from ra_amd.shell import RaShell


def elect(sh, G, N):
    for g in range(G):
        sh.trigger_election(g, g % N)
    sh.run_until_quiet()
    assert [sh.leader_of(g) for g in range(G)] == [g % N for g in range(G)]


def settle(sh):
    sh.run_until_quiet()
    sh.tick_leaders()                                                  # the last commit index reaches the followers
    sh.run_until_quiet()


def put_everywhere(sh, G, want, key):
    for g in range(G):
        assert sh.command(g, ("put", key, g)), g
        want[g][key] = g
    settle(sh)


def assert_machines_agree(sh, G, N, want):
    for g in range(G):
        for slot in range(N):
            s = g * N + slot
            if s in sh.down:
                continue
            assert sh.machines[s].state == want[g], (g, slot, sh.machines[s].state, want[g])


def transfer_loop(eng, G, N):
    eng.set_state(0, abi.empty_server_states(G, N))
    sh = RaShell(eng, G, N)
    elect(sh, G, N)
    want = [dict() for _ in range(G)]
    put_everywhere(sh, G, want, "a")
    # every group moves its leadership to an up-to-date member
    terms = [int(sh.state[g * N + sh.leader_of(g)]["current_term"]) for g in range(G)]
    targets = [(sh.leader_of(g) + 1 + g % (N - 1)) % N for g in range(G)]
    calls = [sh.transfer_leadership(g, targets[g]) for g in range(G)]
    sh.run_until_quiet()
    assert [c.reply for c in calls] == ["ok"] * G
    for g in range(G):
        assert sh.leader_of(g) == targets[g], g
        assert int(sh.state[g * N + targets[g]]["current_term"]) > terms[g], g
        assert all(int(sh.state[g * N + k]["role"]) == abi.ROLE_FOLLOWER for k in range(N) if k != targets[g]), g
    put_everywhere(sh, G, want, "b")                                   # the new leaders commit
    assert_machines_agree(sh, G, N, want)
    # the calls that fail leave the leader where it is
    lead = sh.leader_of(0)
    assert sh.transfer_leadership(0, lead).reply is None              # (answered by the next tick)
    sh.run_until_quiet()
    c1, c2 = sh.transfer_leadership(0, lead), sh.transfer_leadership(1, None)
    sh.run_until_quiet()
    assert (c1.reply, c2.reply) == ("already_leader", ("error", "unknown_member"))
    assert sh.leader_of(0) == lead
    # a target cut off: the old leader stays in the condition until the timeout returns it to leader
    lead = sh.leader_of(0)
    cut = (lead + 1) % N
    sh.partition(0, cut)
    call = sh.transfer_leadership(0, cut)
    sh.run_until_quiet()
    assert call.reply == "ok"
    assert int(sh.state[lead]["role"]) == abi.ROLE_AWAIT_CONDITION
    assert int(sh.state[lead]["cond_reason"]) == abi.COND_TRANSFER_LEADERSHIP
    assert sh.leader_of(0) is None and not sh.command(0, ("put", "lost", 0))
    sh.await_condition_timeouts()
    sh.run_until_quiet()
    assert sh.leader_of(0) == lead and int(sh.state[lead]["cond_reason"]) == abi.COND_NONE
    put_everywhere(sh, G, want, "c")                                   # it commits again (a majority is up)
    assert_machines_agree(sh, G, N, want)
    sh.heal(0, cut)
    # drain: no group is led from member slot `slot` any more
    slot = sh.leader_of(1)
    ticks0 = sh.ticks
    drained = drain(sh, G, N, slot)
    assert drained > 0 and sh.ticks > ticks0
    assert all(sh.leader_of(g) != slot for g in range(1, G)), [sh.leader_of(g) for g in range(G)]
    put_everywhere(sh, G, want, "d")
    assert_machines_agree(sh, G, N, want)
    return sh


def drain(sh, G, N, slot):
    """Move every leader off member slot `slot` (to the next slot); returns how many groups moved."""
    calls = [sh.transfer_leadership(g, (slot + 1) % N) for g in range(G) if sh.leader_of(g) == slot]
    sh.run_until_quiet()
    assert all(c.reply == "ok" for c in calls), [c.reply for c in calls]
    return len(calls)


@pytest.mark.parametrize("G,N", [(8, 3), (6, 5)])
def test_transfer_leadership_closed_loop_on_the_emulated_engine(emulated_engine, G, N):
    with emulated_engine.RaGpuBatch(G, N, ring_capacity=G * N, ring_slots=2, max_runs=8) as eng:
        transfer_loop(eng, G, N)


@pytest.mark.gpu
def test_transfer_leadership_closed_loop_on_the_gpu():
    """4096 groups of five: every group transfers at once (a batch of thousands of transfers, the drain's shape)."""
    from ra_amd import engine
    G, N = 4096, 5
    with engine.RaGpuBatch(G, N, ring_capacity=G * N, ring_slots=2, max_runs=8) as eng:
        transfer_loop(eng, G, N)
