"""The 2-D side of the verification pipeline: float64 ideal model, fixed model, comparison."""
