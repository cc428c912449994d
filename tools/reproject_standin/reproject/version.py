version = "0.0.standin"
