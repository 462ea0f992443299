"""components._PlanCache: the policy both file-backed lift predictors share - stream at first sight, invert at second sight, keep the
most recently used plans, bound the record of keys seen once.  Pure Python: the plans here are strings."""
from interactvlm_amd.components import _PlanCache


def _builder(log, key):
    def build():
        log.append(key)
        return f"plan-{key}"
    return build


def sight(cache, log, key):
    return cache.plan_for(key, _builder(log, key))


def test_first_sight_streams_second_builds_then_the_plan_is_kept():
    cache, log = _PlanCache(2), []
    assert sight(cache, log, "a") is None and log == [] and len(cache) == 0
    assert sight(cache, log, "a") == "plan-a" and log == ["a"] and len(cache) == 1
    assert sight(cache, log, "a") == "plan-a" and log == ["a"]
    assert cache.get("a") == "plan-a" and cache.get("b") is None


def test_a_key_without_identity_always_streams_and_leaves_no_record():
    cache, log = _PlanCache(2), []
    for _ in range(3):
        assert sight(cache, log, None) is None
    assert log == [] and len(cache) == 0 and len(cache._seen_once) == 0


def test_eviction_is_least_recently_used_and_a_hit_refreshes():
    cache, log = _PlanCache(2), []
    for key in "aabb":
        sight(cache, log, key)
    assert sight(cache, log, "a") == "plan-a"  # a hit: b is now the least recently used
    sight(cache, log, "c")
    assert sight(cache, log, "c") == "plan-c" and len(cache) == 2
    assert cache.get("b") is None and cache.get("a") == "plan-a" and cache.get("c") == "plan-c"
    # an evicted key starts over: streamed once, inverted again at the sight after that
    assert sight(cache, log, "b") is None and log == ["a", "b", "c"]
    assert sight(cache, log, "b") == "plan-b" and log == ["a", "b", "c", "b"]
    assert cache.get("a") is None and len(cache) == 2  # (get above refreshed a, then c: a was the oldest)


def test_the_seen_once_record_is_bounded_oldest_first():
    cache, log = _PlanCache(2, seen_capacity=3), []
    for key in "abcd":
        assert sight(cache, log, key) is None
    assert list(cache._seen_once) == ["b", "c", "d"]
    assert sight(cache, log, "a") is None          # forgotten: a first sight again (and b falls out)
    assert sight(cache, log, "d") == "plan-d" and "d" not in cache._seen_once
    assert log == ["d"]
