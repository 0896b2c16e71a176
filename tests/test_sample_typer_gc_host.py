"""cohort.SampleTyper keeps the process's long-lived objects out of the garbage collector's generations while samples are
typed (a full collection would walk the whole index behind the interpreter lock) and hands them back when it is closed."""
import gc

from kir_graph_amd import cohort


def test_long_lived_objects_are_frozen_while_a_typer_is_open():
    gc.unfreeze()
    keep = [[i] for i in range(1000)]      # tracked containers that exist before the typer does
    assert gc.get_freeze_count() == 0
    with cohort.SampleTyper("full", lanes=1) as typer:
        assert gc.get_freeze_count() >= len(keep)
        assert typer.inFlight() == 0
    assert gc.get_freeze_count() == 0 and len(keep) == 1000
    typer.close()                          # closing twice is harmless
    assert gc.get_freeze_count() == 0
