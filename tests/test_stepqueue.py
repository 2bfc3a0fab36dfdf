"""stepqueue.StepPlans: the one place that decides whether a step is replayed from a plan or performed entry by entry
(SubdomainRunner.step, controller.LocalGroup.step, SlabSim.step)."""
from sailfish_amd.stepqueue import DirectQueue, NotPlannable, StepPlans


class FakePlan(object):
    planned = True

    def __init__(self, calls):
        self.calls = calls

    def run(self, it):
        self.calls.append(('run', self, it))


class FakeBackend(object):
    def __init__(self):
        self.calls = []

    def make_plan(self):
        plan = FakePlan(self.calls)
        self.calls.append(('make_plan', plan))
        return plan

    def set_iteration(self, it):
        self.calls.append(('set_iteration', self, it))


def make(enabled=True):
    b = FakeBackend()

    def program(q):
        b.calls.append(('program', q))
    return b, StepPlans(b, enabled), program


def test_a_plan_is_recorded_once_and_replayed():
    b, plans, program = make()
    assert plans.run('k', 4, program, [b]) is True
    plan = plans.plans['k']
    assert b.calls == [('make_plan', plan), ('program', plan), ('run', plan, 4)]
    del b.calls[:]
    assert plans.run('k', 6, program, [b]) is True
    assert b.calls == [('run', plan, 6)]                   # not recorded again
    assert plans.run('other', 7, program, [b]) is True and sorted(plans.plans) == ['k', 'other']


def test_a_program_that_cannot_be_planned_runs_direct_and_ends_planning():
    b, plans, _ = make()
    seen = []

    def program(q):
        seen.append(q)
        if q.planned:
            raise NotPlannable('needs Python')
    assert plans.run('k', 0, program, [b]) is False
    assert [type(q) for q in seen] == [FakePlan, DirectQueue]           # direct in that same call
    assert plans.plans == {} and plans.enabled is False
    del seen[:], b.calls[:]
    for key in ('k', 'other'):
        assert plans.run(key, 1, program, [b]) is False
    assert [type(q) for q in seen] == [DirectQueue, DirectQueue] and plans.plans == {}
    assert not [c for c in b.calls if c[0] == 'make_plan']              # never planned again, for any key


def test_a_step_that_may_not_use_a_plan_leaves_the_plans_alone():
    b, plans, program = make()
    plans.run('k', 0, program, [b])
    plan = plans.plans['k']
    del b.calls[:]
    assert plans.run('k', 2, program, [b], may_plan=False) is False
    assert [c[0] for c in b.calls] == ['set_iteration', 'program'] and isinstance(b.calls[1][1], DirectQueue)
    assert plans.plans == {'k': plan} and plans.enabled is True
    assert plans.run('new', 3, program, [b], may_plan=False) is False and sorted(plans.plans) == ['k']
    del b.calls[:]
    assert plans.run('k', 4, program, [b]) is True
    assert b.calls == [('run', plan, 4)]


def test_only_the_direct_path_sets_the_iteration():
    b, plans, program = make(enabled=False)
    other = FakeBackend()
    other.calls = b.calls
    assert plans.run('k', 5, program, [b, other]) is False
    assert b.calls[:2] == [('set_iteration', b, 5), ('set_iteration', other, 5)] and b.calls[2][0] == 'program'
    assert len(b.calls) == 3 and b.calls[2][1].backend is b
    b, plans, program = make()
    plans.run('k', 5, program, [b, b])
    plans.run('k', 7, program, [b, b])
    assert not [c for c in b.calls if c[0] == 'set_iteration']
