"""Drop-in for the reference's src/evaluation package: eval_suite scores on the MI355X (diner_amd.evaluate)."""
