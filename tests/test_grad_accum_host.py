"""Gradient accumulation, host side (no GPU): the index arithmetic of train_entry.micro_batch_indices — which samples micro-batch i of optimiser step `update` holds on
one rank — over one epoch, and the argument path (TrainingArguments.gradient_accumulation_steps > 1 gets past train()'s argument checks)."""
import itertools

import pytest


@pytest.mark.parametrize("world,GA,B", list(itertools.product((1, 2), (1, 2, 3), (1, 4))))
def test_micro_batch_indices_partition_an_epoch(world, GA, B):
    from llava_mi355x.train_entry import micro_batch_indices
    n = 53                                                        # not a multiple of anything above: the tail of the epoch is dropped
    order = [(7 * i + 3) % n for i in range(n)]                   # a permutation (7 and 53 are coprime)
    updates = (n // (B * world)) // GA
    assert updates >= 1
    seen, per_rank = [], {r: [] for r in range(world)}
    for u in range(updates):
        for i in range(GA):
            for r in range(world):
                idx = micro_batch_indices(order, u, i, r, world, B, GA)
                assert len(idx) == B
                seen += idx; per_rank[r] += idx
                if GA == 1:
                    assert idx == order[(u * world + r) * B:][:B]           # the walk without accumulation
    assert len(seen) == len(set(seen)) == updates * GA * world * B           # no sample twice
    for a, b in itertools.combinations(range(world), 2):
        assert not set(per_rank[a]) & set(per_rank[b])                       # ranks are disjoint
    assert seen == order[:len(seen)]                                         # consecutive groups of world x B, in micro-batch order: nothing skipped inside the epoch


def test_gradient_accumulation_steps_pass_the_argument_checks():
    """train() reads gradient_accumulation_steps first: 2 goes on to the next thing it reads (the model arguments: a stub that stops the call there), 0 is refused."""
    from llava_mi355x import train_data as D, train_entry as E

    class Reached(Exception):
        pass

    class StopAtVersion:
        @property
        def version(self):
            raise Reached()

    args = D.TrainingArguments(gradient_accumulation_steps=2)
    assert args.gradient_accumulation_steps == 2
    with pytest.raises(Reached):
        E.train(StopAtVersion(), None, args, config=None, weights={}, tokenizer=None)
    with pytest.raises(ValueError, match="gradient_accumulation_steps"):
        E.train(StopAtVersion(), None, D.TrainingArguments(gradient_accumulation_steps=0), config=None, weights={}, tokenizer=None)
