"""The walk-skip backoff rule (include/gamdp.h, gamdp_ctx_set_walk_skip_backoff) as ten lines of Python: what one walk does with the
outcomes its candidate points would have under GAMDP_WALK_BACKOFF_OFF.  `hold_of` is the schedule -- the tests hand in the library's own
gamdp_walk_skip_backoff_hold, so nothing here knows the cap."""


def simulate(outcomes, hold_of):
    """outcomes: per candidate point, whether a test there skips at least one group -> (tests made, points held)"""
    fails = hold = tests = held = 0
    for passed in outcomes:
        if hold > 0:
            hold -= 1
            held += 1
            continue
        tests += 1
        fails = 0 if passed else fails + 1
        hold = 0 if passed else hold_of(fails)
    return tests, held
